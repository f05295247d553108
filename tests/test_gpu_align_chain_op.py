"""GPU op tests of the alignment chain's kernels (csrc/kernels_align.hip) one stage at a time: the probabilities of every key kind
against float64 (wm_op_align_probs), the normalised matrix M against the CPU restatement bit for bit (wm_op_align_norm), and the DTW
at the sizes where its code changes path (wm_op_token_times, wm_op_token_times_rows).  The operands, tables and references come from
tests/test_align_tables.py, which also proves on the CPU that they still hold the edges they are there for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_align_tables as gen
from test_token_timestamps import normalise, restate_times

pytestmark = pytest.mark.gpu

SENTINEL = gen.SENTINEL
WM_E_ARG = -1
ALIGN_MAX_ROWS = 447
KV_DTYPE = {"f32": 0, "bf16": 1, "f16": 2}


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from whisper_mojo_amd import _lib
    return _lib.lib()


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run_probs(c, prob, probs=None):
    """wm_op_align_probs on a generated problem; probs defaults to a sentinel-filled buffer."""
    from whisper_mojo_amd import whisper_tensor as wt
    if probs is None:
        probs = np.full((c["B"], c["n_sel"], c["L"], c["T"]), SENTINEL, np.float32)
    keys = dict(X=prob["X"], Wk=prob["Wk"]) if c["kind"] == "absorbed" else dict(kv=prob["kv"], kv_dtype=KV_DTYPE[c["kind"]])
    return wt.align_probs(prob["q"], prob["pairs"], np.asarray(c["rows"], np.int32), c["n_layers"], probs=probs, **keys)


@pytest.mark.parametrize("c", gen.PROBS_CASES, ids=gen.case_id)
def test_align_probs_vs_float64(hip, c):
    """align_kh / align_scores<T> / align_softmax against softmax_j(0.125·q_r·K_j) in float64 on the operands as the kernels see them
    (K rounded to the cache type; absorbed: K_h = bf16(X)·bf16(Wk_h)ᵀ, no bias).  The bar is max(1e-6, 4·e32), e32 being the deviation
    of the same chain in numpy float32 from that reference on this very case: 1e-6 is what test_capture_kat_micro_fp32 asks of the
    probabilities, the factor 4 covers another summation order and expf against numpy's exp.  A wrong layer, head, batch or K/V offset
    lands on a block of another scale (or on the V half's large numbers) and moves probabilities by 1e-2 or more."""
    prob = gen.probs_problem(c)
    ref64, ref32 = gen.probs_refs(c, prob)
    got = run_probs(c, prob)
    live = np.zeros(got.shape, bool)
    for b, R in enumerate(c["rows"]):
        live[b, :, :R] = True
    e32 = float(np.abs(ref32 - ref64).max())
    bar = max(1e-6, 4 * e32)
    assert np.isfinite(got[live]).all()
    dev = float(np.abs(np.where(live, got, 0) - ref64).max())
    sums = np.where(live, got, 0).sum(-1, dtype=np.float64)[live.any(-1)]
    sum_dev = float(np.abs(sums - 1).max()) if sums.size else 0.0
    print(f"align_probs {gen.case_id(c)}: gpu dev {dev:.3e}  e32 {e32:.3e}  bar {bar:.3e}  max |row sum - 1| {sum_dev:.3e}")
    # measured on an MI355X, the largest gpu dev of each key kind / that case's e32: f32 4.77e-6 / 4.80e-6 (d 384, L 130, T 65), bf16
    # 3.35e-6 / 3.40e-6 (d 384, T 1500), f16 4.87e-6 / 4.90e-6 (d 128, L 130, T 65), absorbed 6.13e-6 / 6.16e-6 (d 128, L 130, T 65); the
    # largest ratio is 1.6: absorbed d 512, T 1500, 3.47e-6 against 2.15e-6.  Both chains share the fp32 rounding of the +60 scores.
    assert dev <= bar
    assert sum_dev <= bar
    np.testing.assert_array_equal(_bits(got[~live]), _bits(np.full(int((~live).sum()), SENTINEL)))  # rows >= rows[b]: never written
    np.testing.assert_array_equal(_bits(run_probs(c, prob)), _bits(got))  # a second call: the same bits


@pytest.mark.parametrize("kind", ["bf16", "absorbed"])
def test_align_probs_rows_and_utterances_are_independent(hip, kind):
    """An utterance alone (B = 1, L = its own row count) and the same utterance inside a B = 3 call with a larger L: the same bits.
    Nothing an utterance's probabilities are made of may depend on the batch around it or on the row capacity."""
    c = dict(kind=kind, d=384, n_layers=2, n_sel=3, rows=(65, 130, 7), B=3, L=130, T=257)
    prob = gen.probs_problem(c, seed=4242)
    full = run_probs(c, prob)
    for b, R in enumerate(c["rows"]):
        c1 = dict(c, rows=(R,), B=1, L=R)
        p1 = dict(pairs=prob["pairs"], q=np.ascontiguousarray(prob["q"][b:b + 1, :R]))
        if kind == "absorbed":
            p1.update(X=prob["X"][b:b + 1], Wk=prob["Wk"])
        else:
            p1.update(kv=np.ascontiguousarray(prob["kv"][:, :, b:b + 1]))
        alone = run_probs(c1, p1)
        assert np.isfinite(alone).all() and alone.shape == (1, 3, R, 257)
        np.testing.assert_array_equal(_bits(alone[0]), _bits(full[b, :, :R]), err_msg=f"utterance {b}")


def nan_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


@pytest.mark.parametrize("name", sorted(gen.NORM_LAUNCHES))
def test_align_norm_equals_restatement(hip, name):
    """align_stats / align_median against test_token_timestamps.normalise, bit for bit, NaNs at equal places: the restatement's claim
    to be the kernels' arithmetic operation for operation, which the times comparisons lean on but cannot see (an error in an edge
    column of M need not move the DTW path).  One ragged launch per case; outside each table's R_b x F_b corner the sentinel stays."""
    from whisper_mojo_amd import whisper_tensor as wt
    tabs, packed, R, F = gen.norm_launch(name)
    M = np.full((len(tabs),) + packed.shape[2:], SENTINEL, np.float32)
    wt.align_norm(packed, R, F, M=M)
    n_nan = 0
    for i, w in enumerate(tabs):
        want = np.full(M.shape[1:], SENTINEL, np.float32)
        if R[i]:
            want[:R[i], :F[i]] = normalise(w)
        n_nan += int(np.isnan(want).sum())
        assert nan_equal(M[i], want), f"{name} table {i} ({R[i]} x {F[i]}): " \
            f"{int((~((M[i] == want) | (np.isnan(M[i]) & np.isnan(want)))).sum())} cells differ"
    assert n_nan > 0  # every launch holds a constant column or an R = 1 table
    M2 = np.full_like(M, SENTINEL)
    wt.align_norm(packed, R, F, M=M2)
    np.testing.assert_array_equal(_bits(M2), _bits(M))


def lds_trace_limit():
    """ALIGN_LDS_MAX as csrc/kernels_align.hip states it (bytes)."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "whisper.mojo_amd", "csrc", "kernels_align.hip")).read()
    m = re.search(r"ALIGN_LDS_MAX\s*=\s*(\d+)\s*\*\s*1024\s*;", src)
    assert m, "ALIGN_LDS_MAX is no longer written as N * 1024"
    return int(m.group(1)) * 1024


def test_dtw_trace_boundary_is_where_these_tests_think():
    """align_dtw_lds_bytes(L, 1500) = 3·(L + 1)·4 + L·ceil(1500 / 16)·4 = 388·L + 12 against ALIGN_LDS_MAX = 150 KiB: L = 395 is the
    last trace in LDS, 396 the first in global memory.  If the constant or the formula's inputs move, this fails instead of
    test_dtw_vs_restatement_at_the_edges silently covering one path only."""
    limit = lds_trace_limit()
    assert limit == 150 * 1024
    assert 3 * (395 + 1) * 4 + 395 * ((1500 + 15) // 16) * 4 == 388 * 395 + 12
    assert 388 * 395 + 12 <= limit < 388 * 396 + 12
    assert (395, 1500) in gen.DTW_SHAPES and (396, 1500) in gen.DTW_SHAPES and (ALIGN_MAX_ROWS, 1500) in gen.DTW_SHAPES


def times_alone(hip, w, n_prompt):
    from whisper_mojo_amd import _lib
    n_sel, R, F = w.shape
    out = np.full(n_prompt + R + 1, -7.0, np.float32)
    _lib.check(hip.wm_op_token_times(_fp(out), _fp(np.ascontiguousarray(w)) if R else None, n_sel, R, F, n_prompt))
    return out


def times_rows(hip, packed, R, F, row0, stride):
    from whisper_mojo_amd import _lib
    n_tab, n_sel, L, T = packed.shape
    out = np.full((n_tab, stride), -7.0, np.float32)
    _lib.check(hip.wm_op_token_times_rows(_fp(out), _fp(packed), n_tab, n_sel, L, T, _ip(np.asarray(R, np.int32)), _ip(np.asarray(F, np.int32)),
                                          _ip(np.asarray(row0, np.int32)), stride))
    return out


@pytest.mark.parametrize("kind,R,F", gen.dtw_cases(), ids=lambda v: str(v))
def test_dtw_vs_restatement_at_the_edges(hip, kind, R, F):
    """wm_op_token_times and wm_op_token_times_rows against restate_times, exactly: a second wave of align_dtw (R >= 64), the 16-column
    trace word (F 16 / 17), the last LDS trace and the first global one (395 / 396 x 1500), ALIGN_MAX_ROWS, R > F, tables whose costs
    tie all the time, and tables with NaN columns."""
    w = gen.dtw_table(kind, R, F)
    want = gen.dtw_want(kind, R, F)
    assert kind == "nan" or R >= F or len(set(want[:R])) > 1  # the path does move (NaN costs and R >= F pin it to one column)
    np.testing.assert_array_equal(times_alone(hip, w, 0), want)
    got = times_rows(hip, w[None], [R], [F], [4], R + 7)[0]
    full = np.zeros(R + 7, np.float32)
    full[4:4 + R + 1] = want
    np.testing.assert_array_equal(got, full)


def test_dtw_ragged_launch_vs_restatement(hip):
    """One launch under L = 130, T = 256 that mixes R_b in {0, 1, 64, 130}, row0 in {1, 4, 9} and F_b in {17, 100, 256}."""
    specs = [(130, 256, 1), (0, 100, 4), (64, 17, 9), (1, 256, 4), (64, 100, 1), (130, 17, 9), (1, 17, 1), (130, 100, 4), (64, 256, 9)]
    tabs = [gen.prob_table(9500 + i, 2, R, F, const=i in (4, 7)) for i, (R, F, _) in enumerate(specs)]
    packed = np.full((len(specs), 2, 130, 256), np.nan, np.float32)
    for i, w in enumerate(tabs):
        packed[i, :, :w.shape[1], :w.shape[2]] = w
    stride = 9 + 130 + 1 + 2
    got = times_rows(hip, packed, [s[0] for s in specs], [s[1] for s in specs], [s[2] for s in specs], stride)
    for i, (R, F, row0) in enumerate(specs):
        want = np.zeros(stride, np.float32)
        want[:row0 + R + 1] = restate_times(tabs[i], row0)
        np.testing.assert_array_equal(got[i], want, err_msg=f"table {i}: {R} x {F}, row0 {row0}")
        np.testing.assert_array_equal(times_alone(hip, tabs[i], row0), want[:row0 + R + 1], err_msg=f"table {i} alone")


def test_align_hooks_refuse_bad_arguments(hip):
    """WM_E_ARG, and the output buffers keep every bit."""
    B, L, n_sel, T, d, nl = 2, 4, 2, 8, 128, 2
    q = np.ones((B, L, n_sel, 64), np.float32)
    kv = np.ones((nl, 2, B, T, d), np.float32)
    X, Wk = np.ones((B, T, d), np.float32), np.ones((nl, 2, d, d), np.float32)
    pairs = np.asarray([[0, 0], [1, 1]], np.int32)
    rows = np.asarray([4, 2], np.int32)
    big = max(ALIGN_MAX_ROWS + 1, 33)
    probs = np.full((B, 33, big, T), SENTINEL, np.float32)  # large enough for every shape asked for below, were one to run

    def call(**kw):
        a = dict(probs=_fp(probs), q=_fp(q), kv=_fp(kv), kv_dtype=1, X=None, Wk=None, pairs=_ip(pairs), n_sel=n_sel, rows=_ip(rows), B=B, L=L,
                 T=T, d=d, nl=nl)
        a.update(kw)
        return hip.wm_op_align_probs(a["probs"], a["q"], a["kv"], a["kv_dtype"], a["X"], a["Wk"], a["pairs"], a["n_sel"], a["rows"], a["B"],
                                     a["L"], a["T"], a["d"], a["nl"])

    def ints(*v):
        return _ip(np.asarray(v, np.int32))
    bad_probs = [dict(n_sel=0), dict(n_sel=33), dict(L=0), dict(L=ALIGN_MAX_ROWS + 1), dict(d=96), dict(d=0), dict(T=0), dict(B=0), dict(nl=0),
                 dict(rows=ints(5, 2)), dict(rows=ints(4, -1)), dict(pairs=ints(2, 0, 1, 1)), dict(pairs=ints(0, 0, 1, 2)),
                 dict(pairs=ints(-1, 0, 1, 1)), dict(pairs=ints(0, -1, 1, 1)), dict(probs=None), dict(q=None), dict(pairs=None), dict(rows=None),
                 dict(kv=None), dict(kv=None, X=_fp(X)), dict(kv=None, Wk=_fp(Wk)), dict(X=_fp(X), Wk=_fp(Wk)), dict(kv_dtype=3)]
    for kw in bad_probs:
        assert call(**kw) == WM_E_ARG, kw
        assert hip.wm_last_error()
    assert (_bits(probs) == _bits(SENTINEL)).all()
    assert call() == 0 and call(kv=None, X=_fp(X), Wk=_fp(Wk)) == 0  # the same arguments, unbroken, are accepted
    assert np.isfinite(probs.ravel()[:B * n_sel * L * T]).any()

    n_tab, Ln, Tn = 2, 3, 8
    w = np.full((n_tab, 33, big, Tn), 0.5, np.float32)
    M = np.full((n_tab, big, Tn), SENTINEL, np.float32)

    def norm(**kw):
        a = dict(M=_fp(M), w=_fp(w), n_tab=n_tab, n_sel=2, L=Ln, T=Tn, R=ints(3, 1), F=ints(8, 4))
        a.update(kw)
        return hip.wm_op_align_norm(a["M"], a["w"], a["n_tab"], a["n_sel"], a["L"], a["T"], a["R"], a["F"])
    for kw in [dict(n_sel=0), dict(n_sel=33), dict(L=0), dict(L=ALIGN_MAX_ROWS + 1), dict(T=0), dict(n_tab=0), dict(R=ints(4, 1)),
               dict(R=ints(3, -1)), dict(F=ints(9, 4)), dict(F=ints(8, 0)), dict(M=None), dict(w=None), dict(R=None), dict(F=None)]:
        assert norm(**kw) == WM_E_ARG, kw
    assert (_bits(M) == _bits(SENTINEL)).all()
    assert norm() == 0
    assert not (_bits(M.ravel()[:n_tab * Ln * Tn]) == _bits(SENTINEL)).all()
