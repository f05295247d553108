"""End-to-end tests (-m gpu) of wm_score / wm_score_submit / wm_score_wait / wm_score_pcm.

Against the HF fixtures of tools/make_golden_score.py (fp32, micro and tiny): |logprob - HF|, |sum / n - HF mean| and
|avg + HF loss| <= 1e-4 — the log-prob bar of tests/test_gpu_logprobs.py, for the reason stated there (a log-prob is the difference
of two quantities each within the project's 5e-5 fp32 logits bar).  The 16-bit models are checked for sanity and invariance here;
their arithmetic guarantee is the op test's (tests/test_gpu_score_op.py)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAR = 1e-4
E_ARG, E_STATE = -1, -5


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from whisper_mojo_amd import _lib
    _lib.lib()
    import whisper_mojo_amd as pkg
    return pkg


_CACHE = {}


def setup(name):
    if name not in _CACHE:
        from whisper_mojo_amd import WhisperConfig, synth
        cfg = WhisperConfig.micro() if name == "micro" else WhisperConfig.tiny()
        z = np.load(os.path.join(GOLDEN, f"score_{name}_hf.npz"))
        rows = []
        for i in range(int(z["n_rows"])):
            k = f"r{i}_"
            rows.append(dict(case=str(z[k + "case"]), seed=int(z[k + "seed"]), ids=z[k + "ids"].tolist(), ctx=int(z[k + "context_len"]),
                             lps=z[k + "logprobs"], mean=float(z[k + "mean"]), neg_loss=float(z[k + "neg_loss"]), top=z[k + "top_ids"]))
        _CACHE[name] = (cfg, synth.synth_weights(cfg, 0), rows)
    return _CACHE[name]


def _model(cfg, w, max_batch=4, dtype=0, pos_hf=True, coalesce=0):
    from whisper_mojo_amd import GELU_ERF, POS_HF, POS_REF
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    m = Whisper(cfg, compute_dtype=dtype, gelu_mode=GELU_ERF, pos_mode=POS_HF if pos_hf else POS_REF, max_batch=max_batch, coalesce=coalesce)
    m.load(WeightLoader.from_array(w))
    return m


def _mels(cfg, seeds):
    from whisper_mojo_amd import synth
    return np.stack([synth.synth_mel(cfg, s) for s in seeds])


@pytest.mark.parametrize("name", ["micro", "tiny"])
def test_score_matches_hf(hip, name):
    cfg, w, rows = setup(name)
    m = _model(cfg, w, max_batch=4)
    for lo in range(0, len(rows), 4):
        grp = rows[lo:lo + 4]
        lps, (sm, avg), top = m.score(_mels(cfg, [r["seed"] for r in grp]), [r["ids"] for r in grp], [r["ctx"] for r in grp],
                                      return_top_ids=True)
        for b, r in enumerate(grp):
            got = np.asarray(lps[b], np.float64)
            n = len(r["ids"]) - r["ctx"]
            assert len(got) == len(r["ids"]) and got[0] == 0 and top[b][0] == -1
            err = np.abs(got - r["lps"]).max()
            merr, lerr = abs(float(sm[b]) / n - r["mean"]), abs(float(avg[b]) - r["neg_loss"])
            print(f"{name} {r['case']}: len {len(r['ids'])} ctx {r['ctx']} max |logprob - HF| {err:.2e}, |sum/n - mean| {merr:.2e}, "
                  f"|avg + loss| {lerr:.2e}")
            assert err <= BAR and merr <= BAR and lerr <= BAR, (name, r["case"], err, merr, lerr)
            keep = r["top"] >= 0
            np.testing.assert_array_equal(np.asarray(top[b])[keep], r["top"][keep])
    m.close()


@pytest.mark.parametrize("pos_hf", [True, False])
def test_score_reproduces_own_transcription(hip, pos_hf):
    """transcribe_batch(return_logprobs=True) with no suppress lists and no timestamp rules, per-row prompts of different lengths;
    then score its ids with context_len = prompt length: same log-probs within 1e-4, and the score pass's arg-max is the id the greedy
    pass chose wherever the two leading candidates are more than 2e-4 apart (the gap is read from the score pass itself: the same
    prefix scored once more with the arg-max in place of the chosen id)."""
    cfg, w, _ = setup("micro")
    m = _model(cfg, w, max_batch=4, pos_hf=pos_hf)
    mels = _mels(cfg, [9001, 9002, 9003, 9004])
    prompts = [[1, 2, 3], [7, 1, 2, 3], [5] * 17 + [1, 2, 3], [1]]
    ids, (glp, _avg) = m.transcribe_batch(mels, prompts=prompts, return_logprobs=True, eot=900, max_loop=14)
    ctx = [len(p) for p in prompts]
    lps, (_sm, _av), top = m.score(mels, ids, ctx, return_top_ids=True)
    for b in range(4):
        L = ctx[b]
        assert len(ids[b]) > L
        err = np.abs(np.asarray(lps[b][L:], np.float64) - np.asarray(glp[b][L:], np.float64)).max()
        print(f"pos_hf {pos_hf} row {b}: {len(ids[b]) - L} generated ids, max |score - greedy logprob| {err:.2e}")
        assert err <= BAR
        for t in range(L, len(ids[b])):
            if top[b][t] != ids[b][t]:
                alt = ids[b][:t] + [top[b][t]]
                alp, _ = m.score(mels[b:b + 1], [alt], [L])
                gap = alp[0][t] - lps[b][t]
                print(f"  row {b} t {t}: arg-max {top[b][t]} vs chosen {ids[b][t]}, gap {gap:.2e}")
                assert gap <= 2e-4
    m.close()


def _rows_for_invariance(cfg):
    r = np.random.default_rng(5)
    lens = (2, 17, 33, 41)  # 41 ids = 40 inputs: past two prefill chunks of 16
    ids = [r.integers(0, cfg.vocab_size, n).tolist() for n in lens]
    return ids, [1, 3, 1, 20], [9101, 9102, 9103, 9104]


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_score_batch_invariance(hip, dtype):
    """Bitwise: every row alone equals its values in the batch; the batch in a max_batch = 4 model equals the batch in a max_batch = 8
    model.  Every value finite and <= 0 (the tables' tails: test_score_table_tails)."""
    cfg, w, _ = setup("micro")
    ids, ctx, seeds = _rows_for_invariance(cfg)
    mels = _mels(cfg, seeds)
    m = _model(cfg, w, max_batch=4, dtype=dtype)
    lps, (sm, avg), top = m.score(mels, ids, ctx, return_top_ids=True)
    for b in range(4):
        a = np.asarray(lps[b])
        assert np.isfinite(a).all() and (a <= 0).all() and a[0] == 0 and top[b][0] == -1
        assert all(0 <= t < cfg.vocab_size for t in top[b][1:])
        l1, (s1, a1), t1 = m.score(mels[b:b + 1], [ids[b]], [ctx[b]], return_top_ids=True)
        assert l1[0] == lps[b] and t1[0] == top[b], b
        assert s1[0] == sm[b] and a1[0] == avg[b], b
    m.close()
    m8 = _model(cfg, w, max_batch=8, dtype=dtype)
    l8, (s8, a8), t8 = m8.score(mels, ids, ctx, return_top_ids=True)
    assert l8 == lps and t8 == top
    np.testing.assert_array_equal(s8, sm)
    np.testing.assert_array_equal(a8, avg)
    m8.close()


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_score_table_tails(hip, dtype):
    """wm_score's own [B][ids_stride] tables: 0 / -1 at t = 0 and at and past ids_len, with ids_stride larger than every row."""
    from whisper_mojo_amd import _lib
    cfg, w, _ = setup("micro")
    ids, ctx, seeds = _rows_for_invariance(cfg)
    mels = np.ascontiguousarray(_mels(cfg, seeds), np.float32)
    m = _model(cfg, w, max_batch=4, dtype=dtype)
    stride = 50
    tab = np.zeros((4, stride), np.int32)
    for b, r in enumerate(ids):
        tab[b, :len(r)] = r
    lens, cx = np.asarray([len(r) for r in ids], np.int32), np.asarray(ctx, np.int32)
    lps, top = np.full((4, stride), 7.0, np.float32), np.full((4, stride), 7, np.int32)
    sm, avg = np.zeros(4, np.float32), np.zeros(4, np.float32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    f, i = (lambda a: a.ctypes.data_as(fp)), (lambda a: a.ctypes.data_as(ip))
    _lib.check(_lib.lib().wm_score(m._h, mels.ctypes.data_as(C.c_void_p), 0, 4, m.pos_mode, i(tab), i(lens), stride, i(cx), f(lps), i(top), f(sm), f(avg)))
    ref, (rs, ra), rt = m.score(mels, ids, ctx, return_top_ids=True)
    for b in range(4):
        n = lens[b]
        assert lps[b, 0] == 0 and top[b, 0] == -1 and (lps[b, n:] == 0).all() and (top[b, n:] == -1).all()
        assert lps[b, :n].tolist() == ref[b] and top[b, :n].tolist() == rt[b]
        want = np.float32(0)
        for t in range(ctx[b], n):
            want = np.float32(want + lps[b, t])  # the fixed ascending order of score_sums
        assert sm[b] == want == rs[b] and avg[b] == np.float32(want / np.float32(n - ctx[b]))
    m.close()


def test_score_submit_wait_two_slots(hip):
    cfg, w, _ = setup("micro")
    ids, ctx, seeds = _rows_for_invariance(cfg)
    mels = _mels(cfg, seeds)
    m = _model(cfg, w, max_batch=4, coalesce=2)
    want_a = m.score(mels, ids, ctx, return_top_ids=True)
    want_b = m.score(mels[:2], ids[:2], ctx[:2], return_top_ids=True)
    kw = dict(prompt=[1, 2, 3], eot=900, max_loop=14)
    want_t = m.transcribe_batch(mels, **kw)
    m.transcribe_submit(mels, slot=0, **kw)  # coalesce = 2: held for a partner ...
    m.score_submit(mels, ids, slot=1, context_len=ctx)  # ... which a score submit never is: the held pass goes out alone, first
    m.score_submit(mels[:2], ids[:2], slot=2, context_len=ctx[:2])
    got_b = m.score_wait(2, return_top_ids=True)
    got_a = m.score_wait(1, return_top_ids=True)
    assert m.transcribe_wait(0) == want_t
    for got, want in ((got_a, want_a), (got_b, want_b)):
        assert got[0] == want[0] and got[2] == want[2]
        np.testing.assert_array_equal(got[1][0], want[1][0])
        np.testing.assert_array_equal(got[1][1], want[1][1])
    m.close()


def test_transcribe_after_score_is_unchanged(hip):
    cfg, w, _ = setup("micro")
    ids, ctx, seeds = _rows_for_invariance(cfg)
    mels = _mels(cfg, seeds)
    fresh = _model(cfg, w, max_batch=4)
    want = fresh.transcribe_batch(mels, prompt=[1, 2, 3], eot=900, max_loop=14)
    want_rows = fresh.transcribe_batch(mels, prompts=[[1, 2, 3], [1], [4, 1, 2, 3], [1, 2]], eot=900, max_loop=14)
    fresh.close()
    m = _model(cfg, w, max_batch=4)
    m.score(mels, ids, ctx)
    assert m.transcribe_batch(mels, prompt=[1, 2, 3], eot=900, max_loop=14) == want
    m.score(mels, ids, ctx)
    assert m.transcribe_batch(mels, prompts=[[1, 2, 3], [1], [4, 1, 2, 3], [1, 2]], eot=900, max_loop=14) == want_rows
    m.close()


def test_score_error_codes(hip):
    from whisper_mojo_amd import _lib
    cfg, w, _ = setup("micro")
    m = _model(cfg, w, max_batch=2)
    L = _lib.lib()
    mels = np.ascontiguousarray(_mels(cfg, [1, 2, 3]), np.float32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    f, i = (lambda a: a.ctypes.data_as(fp)), (lambda a: a.ctypes.data_as(ip))
    stride = 70
    lps, top = np.zeros((3, stride), np.float32), np.zeros((3, stride), np.int32)
    sm, avg = np.zeros(3, np.float32), np.zeros(3, np.float32)

    def call(B, lens, ctx, tab=None, pos_mode=1, st=stride):
        t = np.ones((3, stride), np.int32) if tab is None else tab
        return L.wm_score(m._h, mels.ctypes.data_as(C.c_void_p), 0, B, pos_mode, i(t), i(np.asarray(lens, np.int32)), st,
                          i(np.asarray(ctx, np.int32)), f(lps), i(top), f(sm), f(avg))

    assert call(2, [5, 5], [1, 1]) == 0
    assert call(2, [1, 5], [1, 1]) == E_ARG                      # ids_len < 2
    assert call(2, [5, cfg.n_text_ctx + 1], [1, 1]) == E_ARG     # ids_len > n_text_ctx
    assert call(2, [5, 9], [1, 1], st=8) == E_ARG                # ids_len > ids_stride
    assert call(2, [5, 5], [0, 1]) == E_ARG                      # context_len < 1
    assert call(2, [5, 5], [1, 5]) == E_ARG                      # context_len > ids_len - 1
    bad = np.ones((3, stride), np.int32)
    bad[1, 3] = cfg.vocab_size
    assert call(2, [5, 5], [1, 1], tab=bad) == E_ARG             # id outside the vocabulary
    bad[1, 3] = -1
    assert call(2, [5, 5], [1, 1], tab=bad) == E_ARG
    assert call(3, [5, 5, 5], [1, 1, 1]) == E_ARG                # B over max_batch
    assert call(2, [5, 5], [1, 1], pos_mode=2) == E_ARG
    # the waits refuse each other's slots, and the pass stays pending for the right one
    toks, n = np.zeros((2, 3 + 1 + 4), np.int32), np.zeros(2, np.int32)
    m.score_submit(mels[:2], [[1, 2, 3, 4], [1, 2, 3]], slot=3)
    assert L.wm_transcribe_wait(m._h, 3, i(toks), i(n)) == E_STATE
    m.score_wait(3)
    m.transcribe_submit(mels[:2], slot=3, prompt=[1, 2, 3], eot=900, max_loop=4)
    assert L.wm_score_wait(m._h, 3, f(lps), i(top), f(sm), f(avg)) == E_STATE
    with pytest.raises(_lib.WhisperMiError):
        m.score_wait(3)  # the Python mirror holds no score record for the slot; the transcribe record is untouched
    m.transcribe_wait(3)
    assert L.wm_score_wait(m._h, 3, f(lps), i(top), f(sm), f(avg)) == E_STATE  # nothing pending
    with pytest.raises(ValueError):
        m.score(mels[:2], [[1, 2], [1]])
    m.close()


def test_score_audio_equals_score_on_log_mel(hip):
    from whisper_mojo_amd import frontend
    cfg, w, _ = setup("micro")
    m = _model(cfg, w, max_batch=2)
    r = np.random.default_rng(3)
    audios = [r.standard_normal(16000).astype(np.float32) * 0.1, r.standard_normal(9000).astype(np.float32) * 0.1]
    ids = [[1, 2, 3, 40, 41, 42, 900], [1, 2, 3, 77]]
    a = frontend.score_audio(m, audios, ids, context_len=3, return_top_ids=True)
    b = m.score(frontend.log_mel(m, audios), ids, context_len=3, return_top_ids=True)
    assert a[0] == b[0] and a[2] == b[2]
    np.testing.assert_array_equal(a[1][0], b[1][0])
    np.testing.assert_array_equal(a[1][1], b[1][1])
    m.close()
