"""End-to-end tests (-m gpu) of n-best scoring: wm_score_nbest and its submit / wait / pcm forms through
Whisper.score_candidates and frontend.score_audio_candidates.

The definition of the feature is the identity with Whisper.score on the clip's mel repeated once per candidate, bit for bit in every
precision configuration (test_equals_score_on_repeated_mel); score itself is pinned to HF by tests/test_gpu_score.py.  The ranking is
checked against the float64 reference of tests/test_nbest_ref.py applied to the RETURNED fp32 sums — the device ranks those very
values, so order and best are exact — and the posterior within the bound derived in tests/test_gpu_nbest_op.py."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_nbest_op import _post_bound
from test_gpu_score import _mels, hip, setup  # noqa: F401
from test_nbest_ref import rank_reference

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -5
PRECISIONS = {
    "fp32": dict(compute_dtype=0),
    "headline": dict(compute_dtype=1, kv_dtype=0, decoder_fp32=True),  # bf16 encoder, fp32 decoder and K/V: the absorbed path
    "bf16_kv": dict(compute_dtype=1),
    "f16_kv": dict(compute_dtype=2),
}
N_CAND = [1, 4, 2]
UTT_OF = [0, 1, 1, 1, 1, 2, 2]
SEEDS = [9201, 9202, 9203]


def _model(cfg, w, max_batch=8, pos_hf=True, coalesce=0, **prec):
    from whisper_mojo_amd import GELU_ERF, POS_HF, POS_REF
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    m = Whisper(cfg, gelu_mode=GELU_ERF, pos_mode=POS_HF if pos_hf else POS_REF, max_batch=max_batch, coalesce=coalesce, **prec)
    m.load(WeightLoader.from_array(w))
    return m


def _candidates(cfg, lmax, seed=0):
    """U = 3 clips with 1, 4 and 2 candidates of different lengths, the longest of lmax + 1 ids (Lmax = lmax inputs), and a context
    length that varies per row -> (candidates per clip, flat rows, flat context lengths)"""
    r = np.random.default_rng(100 * lmax + seed)
    lens = [max(2, lmax + 1 - k) for k in (2, 0, 5, 1, 9, 3, 0)]
    lens[1] = lmax + 1
    flat = [r.integers(0, cfg.vocab_size, n).tolist() for n in lens]
    ctx = [1 + (i % 3) % (n - 1) for i, n in enumerate(lens)]
    cands, k = [], 0
    for n in N_CAND:
        cands.append(flat[k:k + n])
        k += n
    return cands, flat, ctx


def _flat(res, key):
    return [x for d in res for x in d[key]]


def _assert_equals_score(res, ref):
    lps, (sm, avg), top = ref
    assert _flat(res, "token_logprobs") == lps
    assert _flat(res, "top_ids") == top
    got_s, got_a = np.concatenate([d["sum_logprob"] for d in res]), np.concatenate([d["avg_logprob"] for d in res])
    assert np.array_equal(got_s.view(np.uint32), np.asarray(sm).view(np.uint32))
    assert np.array_equal(got_a.view(np.uint32), np.asarray(avg).view(np.uint32))
    assert np.isfinite(got_s).all() and (got_s < 0).all()


@pytest.mark.parametrize("pos_hf", [True, False])
@pytest.mark.parametrize("prec", list(PRECISIONS))
def test_equals_score_on_repeated_mel(hip, prec, pos_hf):
    """Lmax = 3, 16, 17, 20, 33: the last prefill chunk of the pass is P = 3, 16, 1, 4 and 1 (behind full chunks of 16), rows
    left-padded; the reference is score(mel[utt_of], flat ids) on the same model."""
    cfg, w, _ = setup("micro")
    m = _model(cfg, w, pos_hf=pos_hf, **PRECISIONS[prec])
    mels = _mels(cfg, SEEDS)
    for lmax in (3, 16, 17, 20, 33):
        cands, flat, ctx = _candidates(cfg, lmax)
        assert max(len(r) for r in flat) - 1 == lmax
        res = m.score_candidates(mels, cands, context_len=ctx, return_top_ids=True)
        ref = m.score(mels[UTT_OF], flat, ctx, return_top_ids=True)
        _assert_equals_score(res, ref)
    m.close()


def _check_ranking(res, normalize):
    key = np.concatenate([d["avg_logprob" if normalize else "sum_logprob"] for d in res])
    n_cand = [len(d["order"]) for d in res]
    ro, rb, rp = rank_reference(key, n_cand)
    assert _flat(res, "order") == ro.tolist()
    assert [d["best"] for d in res] == rb.tolist() == [d["order"][0] for d in res]
    post = np.concatenate([d["posterior"] for d in res]).astype(np.float64)
    bnd = _post_bound(key, n_cand, rp)
    err = np.abs(post - rp)
    print(f"normalize {normalize}: worst |posterior - float64| / bound {(err / bnd).max():.3g}")
    assert (err <= bnd).all()


@pytest.mark.parametrize("prec", ["fp32", "headline"])
def test_ranking_end_to_end(hip, prec):
    cfg, w, _ = setup("micro")
    m = _model(cfg, w, **PRECISIONS[prec])
    mels = _mels(cfg, SEEDS)
    cands, flat, ctx = _candidates(cfg, 20, seed=1)
    by_sum = m.score_candidates(mels, cands, context_len=ctx)
    by_avg = m.score_candidates(mels, cands, context_len=ctx, normalize=True)
    _check_ranking(by_sum, False)
    _check_ranking(by_avg, True)
    for a, b in zip(by_sum, by_avg):  # the rows themselves do not depend on the key
        assert a["token_logprobs"] == b["token_logprobs"] and np.array_equal(a["sum_logprob"], b["sum_logprob"])
    assert any(a["order"] != b["order"] for a, b in zip(by_sum, by_avg)), "the candidates were chosen so that the two orders differ"
    m.close()


def _same(a, b):
    return (a["token_logprobs"] == b["token_logprobs"] and a["order"] == b["order"] and a["best"] == b["best"]
            and all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in ("sum_logprob", "avg_logprob", "posterior")))


@pytest.mark.parametrize("prec", ["fp32", "headline", "bf16_kv"])
def test_clip_alone_or_in_any_order(hip, prec):
    cfg, w, _ = setup("micro")
    m = _model(cfg, w, **PRECISIONS[prec])
    mels = _mels(cfg, SEEDS)
    cands, flat, ctx = _candidates(cfg, 17)
    cx, k = [], 0
    for n in N_CAND:
        cx.append(ctx[k:k + n])
        k += n
    whole = m.score_candidates(mels, cands, context_len=cx)
    for u in range(3):
        alone = m.score_candidates(mels[u:u + 1], [cands[u]], context_len=[cx[u]])
        assert _same(alone[0], whole[u]), u
    rev = m.score_candidates(mels[::-1], cands[::-1], context_len=cx[::-1])
    for u in range(3):
        assert _same(rev[2 - u], whole[u]), u
    m.close()


@pytest.mark.parametrize("prec", ["fp32", "headline"])
def test_state_reuse_both_ways(hip, prec):
    """The same state (slot 0, 7 rows) serves an n-best pass and then score, transcribe_batch and align — and the reverse order — with
    the bits of a fresh model: the next pass clears the row-to-clip map."""
    cfg, w, _ = setup("micro")
    mels = _mels(cfg, SEEDS)
    cands, flat, ctx = _candidates(cfg, 20)
    mel7 = mels[UTT_OF][::-1].copy()  # seven rows whose clips are NOT what the n-best map would pick
    heads = [(0, 1), (1, 0)]
    kw = dict(prompt=[1, 2, 3], eot=900, max_loop=10)

    def others(m):
        return (m.score(mel7, flat, ctx, return_top_ids=True), m.transcribe_batch(mel7, **kw),
                m.align(mel7, flat, ctx, return_logprobs=True))

    def eq(a, b):
        (s1, t1, a1), (s2, t2, a2) = a, b
        assert s1[0] == s2[0] and s1[2] == s2[2] and np.array_equal(s1[1][0], s2[1][0]) and np.array_equal(s1[1][1], s2[1][1])
        assert t1 == t2
        assert a1[0] == a2[0] and a1[1][0] == a2[1][0]

    fresh = _model(cfg, w, **PRECISIONS[prec])
    fresh.set_alignment_heads(heads)
    want = others(fresh)
    fresh.close()
    fresh = _model(cfg, w, **PRECISIONS[prec])
    want_nb = fresh.score_candidates(mels, cands, context_len=ctx)
    fresh.close()
    m = _model(cfg, w, **PRECISIONS[prec])
    m.set_alignment_heads(heads)
    got_nb = m.score_candidates(mels, cands, context_len=ctx)
    eq(others(m), want)
    again = m.score_candidates(mels, cands, context_len=ctx)
    for a, b, c in zip(got_nb, want_nb, again):
        assert _same(a, b) and _same(c, b)
    eq(others(m), want)
    m.close()


def test_submit_wait_two_slots_and_wait_families(hip):
    from whisper_mojo_amd import _lib
    cfg, w, _ = setup("micro")
    m = _model(cfg, w, coalesce=2, **PRECISIONS["headline"])
    mels = _mels(cfg, SEEDS)
    cands, flat, ctx = _candidates(cfg, 17)
    want_a = m.score_candidates(mels, cands, context_len=ctx, return_top_ids=True)
    want_b = m.score_candidates(mels[:2], cands[:2], context_len=ctx[:5], normalize=True, return_top_ids=True)
    m.score_candidates_submit(mels, cands, slot=1, context_len=ctx)
    m.score_candidates_submit(mels[:2], cands[:2], slot=2, context_len=ctx[:5], normalize=True)
    L = _lib.lib()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    f, i = (lambda a: a.ctypes.data_as(fp)), (lambda a: a.ctypes.data_as(ip))
    lps, top = np.zeros((7, 40), np.float32), np.zeros((7, 40), np.int32)
    sm, avg, post = np.zeros(7, np.float32), np.zeros(7, np.float32), np.zeros(7, np.float32)
    order, best, toks, n = np.zeros(7, np.int32), np.zeros(3, np.int32), np.zeros((7, 40), np.int32), np.zeros(7, np.int32)
    # the other wait families refuse the slot, and the pass stays pending for its own
    assert L.wm_score_wait(m._h, 1, f(lps), i(top), f(sm), f(avg)) == E_STATE
    assert L.wm_transcribe_wait(m._h, 1, i(toks), i(n)) == E_STATE
    assert L.wm_align_wait(m._h, 1, f(lps), None, None, None) == E_STATE
    with pytest.raises(_lib.WhisperMiError):
        m.score_wait(1)
    got_b = m.score_candidates_wait(2, return_top_ids=True)
    got_a = m.score_candidates_wait(1, return_top_ids=True)
    for got, want in ((got_a, want_a), (got_b, want_b)):
        for g, x in zip(got, want):
            assert _same(g, x) and g["top_ids"] == x["top_ids"]
    # ... and the n-best wait refuses a plain score pass, a transcribe pass and an empty slot
    m.score_submit(mels, [r[:4] for r in flat[:3]], slot=3)
    assert L.wm_score_nbest_wait(m._h, 3, f(lps), i(top), f(sm), f(avg), i(order), i(best), f(post)) == E_STATE
    m.score_wait(3)
    m.transcribe_submit(mels, slot=3, prompt=[1, 2, 3], eot=900, max_loop=4)
    assert L.wm_score_nbest_wait(m._h, 3, f(lps), i(top), f(sm), f(avg), i(order), i(best), f(post)) == E_STATE
    m.transcribe_wait(3)
    assert L.wm_score_nbest_wait(m._h, 3, f(lps), i(top), f(sm), f(avg), i(order), i(best), f(post)) == E_STATE
    with pytest.raises(_lib.WhisperMiError):
        m.score_candidates_wait(3)
    m.close()


def test_library_refusals_and_phases(hip):
    from whisper_mojo_amd import _lib
    cfg, w, _ = setup("micro")
    m = _model(cfg, w, max_batch=4)
    L = _lib.lib()
    mels = np.ascontiguousarray(_mels(cfg, SEEDS), np.float32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    f, i = (lambda a: a.ctypes.data_as(fp)), (lambda a: a.ctypes.data_as(ip))
    stride = 8
    lps, top = np.zeros((5, stride), np.float32), np.zeros((5, stride), np.int32)
    sm, avg, post = np.zeros(5, np.float32), np.zeros(5, np.float32), np.zeros(5, np.float32)
    order, best = np.zeros(5, np.int32), np.zeros(3, np.int32)
    tab = np.ones((5, stride), np.int32)

    def call(U, n_cand, lens, ctx=None, pos_mode=1, t=tab):
        return L.wm_score_nbest(m._h, mels.ctypes.data_as(C.c_void_p), 0, U, i(np.asarray(n_cand, np.int32)), 0, pos_mode, i(t),
                                i(np.asarray(lens, np.int32)), stride, i(np.asarray(ctx, np.int32)) if ctx else None, f(lps), i(top), f(sm),
                                f(avg), i(order), i(best), f(post))

    with pytest.raises(_lib.WhisperMiError):
        m.score_phases(0)  # nothing ran yet
    assert call(2, [1, 3], [5, 5, 4, 3]) == 0
    ph = m.score_phases(0)
    assert set(ph) == {"encoder", "prefill", "ln", "sweep", "merge"} and all(v >= 0 for v in ph.values()) and ph["encoder"] > 0
    assert call(0, [1], [5]) == E_ARG                        # U < 1
    assert call(2, [1, 0], [5]) == E_ARG                     # a clip without candidates
    assert call(2, [2, 3], [5] * 5) == E_ARG                 # R over max_batch
    assert call(2, [1, 3], [5, 5, 1, 3]) == E_ARG            # per row, as wm_score: ids_len < 2
    assert call(2, [1, 3], [5, 5, 9, 3]) == E_ARG            # ids_len > ids_stride
    assert call(2, [1, 3], [5, 5, 4, 3], ctx=[1, 1, 4, 1]) == E_ARG
    assert call(2, [1, 3], [5, 5, 4, 3], pos_mode=2) == E_ARG
    bad = tab.copy()
    bad[3, 1] = cfg.vocab_size
    assert call(2, [1, 3], [5, 5, 4, 3], t=bad) == E_ARG
    with pytest.raises(_lib.WhisperMiError):
        m.score_phases(1)
    m.close()


def test_tiny_headline_equals_score(hip):
    """The six-head absorbed instantiation (tiny, bf16 encoder, fp32 decoder and K/V) that the micro model does not reach."""
    from whisper_mojo_amd import WhisperConfig, synth
    cfg = WhisperConfig.tiny()
    w = synth.synth_weights(cfg, 0)
    m = _model(cfg, w, max_batch=6, **PRECISIONS["headline"])
    mels = _mels(cfg, [9301, 9302])
    r = np.random.default_rng(9)
    cands = [[r.integers(0, cfg.vocab_size, n).tolist() for n in grp] for grp in ((10, 7, 11), (9, 10, 4))]
    flat = [c for g in cands for c in g]
    ctx = [1, 3, 2, 1, 4, 2]
    res = m.score_candidates(mels, cands, context_len=ctx, return_top_ids=True)
    ref = m.score(mels[[0, 0, 0, 1, 1, 1]], flat, ctx, return_top_ids=True)
    _assert_equals_score(res, ref)
    _check_ranking(res, False)
    m.close()


def test_audio_candidates_equal_log_mel(hip):
    from whisper_mojo_amd import frontend
    cfg, w, _ = setup("micro")
    m = _model(cfg, w, max_batch=4)
    r = np.random.default_rng(3)
    audios = [r.standard_normal(16000).astype(np.float32) * 0.1, r.standard_normal(9000).astype(np.float32) * 0.1]
    cands = [[[1, 2, 3, 40, 41, 42, 900], [1, 2, 3, 77]], [[1, 2, 3, 5, 6]]]
    a = frontend.score_audio_candidates(m, audios, cands, context_len=3, return_top_ids=True)
    b = m.score_candidates(frontend.log_mel(m, audios), cands, context_len=3, return_top_ids=True)
    for x, y in zip(a, b):
        assert _same(x, y) and x["top_ids"] == y["top_ids"]
    i16 = [(x * 32767).astype(np.int16) for x in audios]
    c = frontend.score_audio_candidates(m, i16, cands, context_len=3)
    d = m.score_candidates(frontend.log_mel(m, i16), cands, context_len=3)
    for x, y in zip(c, d):
        assert _same(x, y)
    # sampling_rate=: resampled to 16 kHz on the GPU first, as every audio entry (8 kHz float and 44.1 kHz int16)
    a8 = [x[::2].copy() for x in audios]
    e = frontend.score_audio_candidates(m, a8, cands, context_len=3, sampling_rate=8000)
    f = m.score_candidates(frontend.log_mel(m, a8, sampling_rate=8000), cands, context_len=3)
    i44 = [(r.standard_normal(n) * 3000).astype(np.int16) for n in (30000, 44100)]
    g = frontend.score_audio_candidates(m, i44, cands, context_len=3, sampling_rate=44100)
    h = m.score_candidates(frontend.log_mel(m, i44, sampling_rate=44100), cands, context_len=3)
    for x, y in list(zip(e, f)) + list(zip(g, h)):
        assert _same(x, y)
    assert not _same(e[0], a[0])  # the 8 kHz clip is another signal: the rate was not ignored
    m.close()
