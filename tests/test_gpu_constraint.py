"""Model-level tests (-m gpu) of the phrase-list constraint on the micro model with synthetic weights.

Reference: the processed greedy loop of tests/test_gpu_seq_bias.py with the numpy restatement of tests/test_constraint_ref.py behind
the other processors — over the CPU oracle for the fp32 model, over the model's own raw logits (wm_decode_step) for the headline
precision.  Ids are compared token for token, no position left out: the recordings are picked, from the oracle alone and before any
GPU run, so that every top-1 margin of the constrained reference streams is at least 4·MARGIN_TOL; log-probs within 1e-4 (§29's bar).
The phrase lists are built from a 12-id alphabet that holds none of the recordings' unconstrained first ids."""
import numpy as np
import pytest

from test_constraint_ref import Table, allowed_ids, process_all, walk_of
from test_gpu_parity import MARGIN_TOL, hip, make_model  # noqa: F401
from test_gpu_repeat import EOT, MAX_LOOP, PROMPT, TS, _headline

pytestmark = pytest.mark.gpu

NP = len(PROMPT)
VOCAB = 1000
# Under the timestamp rules the micro model puts timestamps between the text ids, so a walk of up to six ids needs more steps than
# the 12 of the other files to reach its phrase's end: 40 (17 prompt ids + 1 + 40 fit the 64 decoder positions).
LOOP = {False: MAX_LOOP, True: 40}


def _phrases(alpha, seed):
    """about 40 phrases of 1-6 ids over the alphabet: shared prefixes, phrases that are prefixes of others"""
    r = np.random.default_rng(seed)
    had = []
    while len(had) < 40:
        p = tuple(int(a) for a in r.choice(alpha, int(r.integers(1, 7))))
        for q in (p, p[:int(r.integers(1, len(p) + 1))]):
            if q not in had:
                had.append(q)
    return had


def _step(orc, z, ids, n_prompt, table, ts, opt, suppress=()):
    z = process_all(z, ids, n_prompt, table, **opt)
    z[list(suppress)] = -np.inf
    if ts is not None:
        z[ts[1]] = -np.inf
        z = orc.timestamp_rules(z, ids[n_prompt:], ts[0], ts[1], table.eot, ts[2])
    fin = z.astype(np.float64)[np.isfinite(z)]
    t = int(np.flatnonzero(z == z.max())[0])
    srt = np.sort(fin)
    lp = float(np.float64(z[t]) - (fin.max() + np.log(np.exp(fin - fin.max()).sum()))) if fin.size else -np.inf
    return t, lp, float(srt[-1] - srt[-2]) if fin.size > 1 else np.inf


def _finish(ids, n_prompt, table):
    """constraint_match of a finished reference stream"""
    return allowed_ids(ids[n_prompt:-1], table)[1] if ids[-1] == table.eot else -1


def _ref_stream(orc, om, enc, prompt, table, ts=None, opt={}, suppress=(), max_loop=MAX_LOOP):
    """-> (ids, log-probs, margins, match) of the constrained greedy loop on the CPU oracle"""
    ids, lps, margins = list(prompt), [], []
    for _ in range(max_loop + 1):
        t, lp, mg = _step(orc, om.teacher_forced(enc, ids, n_prompt=len(prompt), pos_mode=0)[-1], ids, len(prompt), table, ts, opt, suppress)
        ids.append(t), lps.append(lp), margins.append(mg)
        if t == table.eot:
            break
    return ids, lps, margins, _finish(ids, len(prompt), table)


def _dev_stream(orc, m, mel, prompt, table, ts=None, opt={}, max_loop=MAX_LOOP):
    """The same loop on the model's own raw logits (no processors, no mask on the device)"""
    from whisper_mojo_amd.whisper import KVCache
    cache = KVCache(m, 1)
    m.encoder.forward(mel, cache)
    z = m.decoder.forward(list(prompt), None, cache, start_pos=0)
    ids, lps, margins = list(prompt), [], []
    for step in range(max_loop + 1):
        t, lp, mg = _step(orc, z, ids, len(prompt), table, ts, opt)
        ids.append(t), lps.append(lp), margins.append(mg)
        if t == table.eot or step == max_loop:
            break
        z = m.decoder.forward([t], None, cache, start_pos=cache.current_len - 1)
    return ids, lps, margins, _finish(ids, len(prompt), table)


@pytest.fixture(scope="module")
def setup(hip):
    """Three recordings, two phrase lists over an alphabet without the recordings' unconstrained first ids, and the oracle's
    constrained streams with the rules off and on — every margin at 4·MARGIN_TOL or more."""
    from oracle import oracle as orc
    from whisper_mojo_amd import WhisperConfig, synth
    cfg = WhisperConfig.micro()
    w = synth.synth_weights(cfg, 0)
    om = orc.OracleModel(cfg, w)
    cand = []
    for seed in range(1001, 1025):
        mel = synth.synth_mels(cfg, seed, 1)[0]
        enc = om.encode(mel)
        first = int(np.argmax(om.teacher_forced(enc, list(PROMPT), n_prompt=NP, pos_mode=0)[-1]))
        cand.append((seed, mel, enc, first))
    firsts = {c[3] for c in cand}
    alpha = [t for t in range(100, 140) if t not in firsts][:12]
    lists = [_phrases(alpha, 1), _phrases(alpha[::-1], 2)]
    assert lists[0] != lists[1] and any(p[:k] in lists[0] for p in lists[0] for k in range(1, len(p)))
    tabs = {(k, ts): Table(lists[k], EOT, TS[0] if ts else None, VOCAB) for k in (0, 1) for ts in (False, True)}
    picked, refs = [], {}
    for seed, mel, enc, first in cand:
        got = {key: _ref_stream(orc, om, enc, PROMPT, t, TS if key[1] else None, max_loop=LOOP[key[1]]) for key, t in tabs.items()}
        if any(v[3] < 0 for v in got.values()):  # (a stream that runs the loop out lands on no phrase: not a recording for these tests)
            continue
        if min(min(v[2]) for v in got.values()) < 4 * MARGIN_TOL:
            continue
        for key, v in got.items():
            refs[(len(picked),) + key] = v
        picked.append((seed, mel, enc, first))
        if len(picked) == 3:
            break
    assert len(picked) == 3
    return cfg, w, orc, om, picked, lists, tabs, refs


def _kw(ts):
    return dict(prompt=PROMPT, eot=EOT, max_loop=LOOP[bool(ts)], **({"timestamps": TS} if ts else {}))


def _mels(setup):
    return np.stack([p[1] for p in setup[4]])


def _same_lp(x, y):
    assert x[0] == y[0] and x[1][0] == y[1][0]
    np.testing.assert_array_equal(np.asarray(x[1][1]).view(np.uint32), np.asarray(y[1][1]).view(np.uint32))
    np.testing.assert_array_equal(x[-1], y[-1])


def test_constraint_confines_the_stream(hip, setup):
    """Every row's generated ids, free ids removed, are one of the phrases followed by eot, constraint_match names that phrase, and
    the unconstrained stream is another one (the phrases hold no row's unconstrained first id)."""
    cfg, w, orc, om, picked, lists, tabs, refs = setup
    m = make_model(cfg, w, max_batch=3)
    for ts in (False, True):
        plain = m.transcribe_batch(_mels(setup), **_kw(ts))
        for k in (0, 1):
            ids, match = m.transcribe_batch(_mels(setup), constraint=lists[k], **_kw(ts))
            assert match.dtype == np.int32 and match.shape == (3,)
            for b in range(3):
                gen = ids[b][NP:]
                assert gen[-1] == EOT, (ts, k, b, gen)
                walk = walk_of(gen[:-1], tabs[(k, ts)])
                assert walk in lists[k] and lists[k].index(walk) == match[b], (ts, k, b, gen, match[b])
                assert ids[b] != plain[b] and picked[b][3] not in walk
                if ts:
                    assert any(t >= TS[0] for t in gen)  # timestamp ids appear, pass through, and the walk still lands on a phrase
    m.close()


@pytest.mark.parametrize("prec", ["fp32", "headline"])
@pytest.mark.parametrize("ts", [False, True], ids=["plain", "timestamps"])
def test_matches_the_processed_loop(hip, setup, ts, prec):
    cfg, w, orc, om, picked, lists, tabs, refs = setup
    m = make_model(cfg, w, max_batch=3) if prec == "fp32" else _headline(cfg, w, 3)
    for k in (0, 1):
        ids, (lps, avg), match = m.transcribe_batch(_mels(setup), return_logprobs=True, constraint=lists[k], **_kw(ts))
        for b, (seed, mel, enc, first) in enumerate(picked):
            if prec == "fp32":
                want, wlp, margins, wmatch = refs[(b, k, ts)]
            else:
                want, wlp, margins, wmatch = _dev_stream(orc, m, mel, PROMPT, tabs[(k, ts)], TS if ts else None, max_loop=LOOP[ts])
            assert ids[b] == want, (prec, seed, k, ids[b], want, min(margins))
            err = np.abs(np.asarray(lps[b][NP:], np.float64) - np.asarray(wlp))
            print(f"{prec} seed {seed} list {k} rules {ts}: {len(want) - NP} positions, max |log-prob error| {err.max():.3g}, match {match[b]}")
            assert (err <= 1e-4).all()
            assert match[b] == wmatch
    m.close()


def test_with_the_other_processors(hip, setup):
    """sequence_bias, repetition_penalty, no_repeat_ngram_size and bad_words_ids ahead of the constraint, in HF's order"""
    cfg, w, orc, om, picked, lists, tabs, refs = setup
    a = sorted({t for p in lists[0] for t in p})
    opt = dict(sequence_bias={(a[0],): 1.0, (a[1], a[2]): -2.0}, bad_words_ids=[[a[3]], [a[4], a[5]]], repetition_penalty=1.3, no_repeat_ngram_size=2)
    ropt = dict(sequence_bias=opt["sequence_bias"], bad_words_ids=opt["bad_words_ids"], p=1.3, n=2)
    m = make_model(cfg, w, max_batch=3)
    ids, (lps, avg), match = m.transcribe_batch(_mels(setup), return_logprobs=True, constraint=lists[0], **opt, **_kw(True))
    for b, (seed, mel, enc, first) in enumerate(picked):
        want, wlp, margins, wmatch = _ref_stream(orc, om, enc, PROMPT, tabs[(0, True)], TS, ropt, max_loop=LOOP[True])
        j = next((i for i in range(min(len(want), len(ids[b]))) if want[i] != ids[b][i]), None)
        assert j is None or margins[j - NP] < MARGIN_TOL, (seed, j, ids[b], want)   # (this table's margins were not part of the pick)
        if j is None:
            assert len(ids[b]) == len(want) and match[b] == wmatch
            assert (np.abs(np.asarray(lps[b][NP:], np.float64) - np.asarray(wlp)) <= 1e-4).all()
        assert not any(t == a[3] for t in ids[b][NP:])
    m.close()


def test_logprobs_and_top_k_see_the_allowed_set(hip, setup):
    cfg, w, orc, om, picked, lists, tabs, refs = setup
    m = make_model(cfg, w, max_batch=3)
    ids, (lps, avg), (ti, tl), match = m.transcribe_batch(_mels(setup), return_logprobs=True, top_k=4, constraint=lists[0], **_kw(True))
    for b in range(3):
        gen = ids[b][NP:]
        np.testing.assert_array_equal(ti[b][:, 0], gen)                       # rank 0 is the emitted id
        for i in range(len(gen)):
            ok = set(allowed_ids(gen[:i], tabs[(0, True)])[0])
            fin = np.isfinite(tl[b][i])
            assert set(ti[b][i][fin].tolist()) <= ok, (b, i)                   # every listed candidate is an allowed id
            assert np.exp(tl[b][i][fin].astype(np.float64)).sum() <= 1 + 1e-5
    m.close()


def test_identities_bit_for_bit(hip, setup):
    """None equals the option absent; B = 3 equals three B = 1 runs; per-row prompts of 1 / 5 / 17 ids equal each row alone; a reused
    state equals a fresh model; four pipelined submits equal the synchronous results."""
    cfg, w, orc, om, picked, lists, tabs, refs = setup
    mels = _mels(setup)
    m = make_model(cfg, w, max_batch=3)
    base = m.transcribe_batch(mels, return_logprobs=True, **_kw(True))
    off = m.transcribe_batch(mels, return_logprobs=True, constraint=None, **_kw(True))
    assert len(off) == 2 and off[0] == base[0] and off[1][0] == base[1][0]
    both = m.transcribe_batch(mels, return_logprobs=True, constraint=lists[0], **_kw(True))
    assert both[0] != base[0]
    for b in range(3):
        one = m.transcribe_batch(mels[b:b + 1], return_logprobs=True, constraint=lists[0], **_kw(True))
        assert one[0][0] == both[0][b] and one[1][0][0] == both[1][0][b] and one[2][0] == both[2][b]
    assert m.transcribe_batch(mels, return_logprobs=True, **_kw(True))[0] == base[0]  # and off again after on
    rows = [[1], [1, 2, 3, 4, 5], list(range(1, 18))]
    kw = dict(eot=EOT, max_loop=LOOP[True], timestamps=TS)
    together, tmatch = m.transcribe_batch(mels, prompts=rows, constraint=lists[0], **kw)
    for b in range(3):
        one, om1 = m.transcribe_batch(mels[b:b + 1], prompts=[rows[b]], constraint=lists[0], **kw)
        assert one[0] == together[b] and om1[0] == tmatch[b]
        gen = together[b][len(rows[b]):]
        assert gen[-1] == EOT and walk_of(gen[:-1], tabs[(0, True)]) == tuple(lists[0][tmatch[b]])   # the walk starts behind the row's own prompt
    again, amatch = m.transcribe_batch(mels[[1, 2, 0]], constraint=lists[0], **_kw(True))
    m.close()
    fresh = make_model(cfg, w, max_batch=3)
    f_ids, f_match = fresh.transcribe_batch(mels[[1, 2, 0]], constraint=lists[0], **_kw(True))
    assert f_ids == again and f_match.tolist() == amatch.tolist()
    assert again == [both[0][1], both[0][2], both[0][0]] and amatch.tolist() == both[2][[1, 2, 0]].tolist()
    for s in range(4):
        fresh.transcribe_submit(mels[[s % 3]], slot=s, constraint=lists[s % 2], **_kw(True))
    for s in range(4):
        got, gm = fresh.transcribe_wait(s)
        if s % 2 == 0:
            assert got[0] == both[0][s % 3] and gm[0] == both[2][s % 3]
        else:
            assert got[0] == refs[(s % 3, 1, True)][0] and gm[0] == refs[(s % 3, 1, True)][3]
    fresh.close()


def test_coalesced_pairs(hip, setup):
    """coalesce = 2: two submits under one table share one 2·B-row state and return the synchronous results; submits under different
    tables are not paired and each follows its own; replacing the table while a submit is held leaves that submit on the old one."""
    cfg, w, orc, om, picked, lists, tabs, refs = setup
    mels = _mels(setup)
    rot = mels[[1, 2, 0]].copy()
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    m = Whisper(cfg, max_batch=3, coalesce=2)
    m.load(WeightLoader.from_array(w))
    kw = dict(return_logprobs=True, **_kw(True))
    want_a, want_b = m.transcribe_batch(mels, constraint=lists[0], **kw), m.transcribe_batch(rot, constraint=lists[0], **kw)
    want_c, plain = m.transcribe_batch(rot, constraint=lists[1], **kw), m.transcribe_batch(rot, **kw)
    assert want_b[0] != want_c[0] and want_b[0] != plain[0]
    m.transcribe_submit(mels, slot=0, constraint=lists[0], **kw)
    m.transcribe_submit(rot, slot=1, constraint=lists[0], **kw)  # the partner: one pass of 6 rows
    _same_lp(m.transcribe_wait(0), want_a)
    _same_lp(m.transcribe_wait(1), want_b)
    m.transcribe_submit(mels, slot=2, constraint=lists[0], **kw)
    m.transcribe_submit(rot, slot=3, constraint=lists[1], **kw)  # another table: no pair, and the held one keeps the one it was asked under
    _same_lp(m.transcribe_wait(2), want_a)
    _same_lp(m.transcribe_wait(3), want_c)
    m.transcribe_submit(mels, slot=2, constraint=lists[0], **kw)
    m.transcribe_submit(rot, slot=3, **kw)                       # a table against none
    _same_lp(m.transcribe_wait(2), want_a)
    got = m.transcribe_wait(3)
    assert len(got) == 2 and got[0] == plain[0]
    m.close()


def test_a_reloaded_model_gets_the_table_again(hip, setup):
    from whisper_mojo_amd.loader import WeightLoader
    cfg, w, orc, om, picked, lists, tabs, refs = setup
    mels = _mels(setup)
    m = make_model(cfg, w, max_batch=3)
    want, wm = m.transcribe_batch(mels, constraint=lists[0], **_kw(False))
    assert want[0] == refs[(0, 0, False)][0]
    m.load(WeightLoader.from_array(w))
    got, gm = m.transcribe_batch(mels, constraint=lists[0], **_kw(False))
    assert got == want and gm.tolist() == wm.tolist()
    m.close()
    m.load(WeightLoader.from_array(w))
    got, gm = m.transcribe_batch(mels, constraint=lists[0], **_kw(False))
    assert got == want and gm.tolist() == wm.tolist()
    m.close()


def test_probe_language_score_and_align_read_raw_logits(hip, setup):
    cfg, w, orc, om, picked, lists, tabs, refs = setup
    mels = _mels(setup)
    m = make_model(cfg, w, max_batch=3)
    kw = dict(return_logprobs=True, no_speech_token=7, **_kw(True))
    a, b = m.transcribe_batch(mels, **kw), m.transcribe_batch(mels, constraint=lists[0], **kw)
    assert a[0] != b[0]
    np.testing.assert_array_equal(np.asarray(a[1][2]).view(np.uint32), np.asarray(b[1][2]).view(np.uint32))
    langs = [10, 11, 12, 13, 14]
    c = m.transcribe_batch(mels, detect_language=langs, **_kw(True))
    d = m.transcribe_batch(mels, detect_language=langs, constraint=lists[0], **_kw(True))
    np.testing.assert_array_equal(c[1][0], d[1][0])
    np.testing.assert_array_equal(np.asarray(c[1][1]).view(np.uint32), np.asarray(d[1][1]).view(np.uint32))
    for bb in range(3):  # detect_language combined with the option: the walk starts behind the filled prompt
        gen = d[0][bb][NP:]
        assert d[0][bb][1] == int(d[1][0][bb]) and gen[-1] == EOT and lists[0].index(walk_of(gen[:-1], tabs[(0, True)])) == d[2][bb]
    # score and align after a pass under the table (the model-wide setting is still in force in the library): unprocessed
    ids = [r[:NP] + [t for t in r[NP:] if t != EOT] for r in a[0]]
    heads = [(cfg.n_layers - 1, 0), (0, cfg.n_heads - 1)]
    s0 = make_model(cfg, w, max_batch=3)
    s0.set_alignment_heads(heads)
    want = s0.score(mels, ids)
    want_t = s0.align(mels, ids, context_len=NP)
    s0.close()
    m.set_alignment_heads(heads)
    m.transcribe_batch(mels, constraint=lists[0], **_kw(False))
    got, got_t = m.score(mels, ids), m.align(mels, ids, context_len=NP)
    for x, y in zip(list(got[0]) + list(got_t), list(want[0]) + list(want_t)):
        np.testing.assert_array_equal(np.asarray(x, np.float32).view(np.uint32), np.asarray(y, np.float32).view(np.uint32))
    m.close()


def test_the_dead_node(hip, setup):
    """suppress_tokens over every child of the root leaves the first step without a finite candidate: the rows emit what the
    reference emits (id 0, then eot from the dead node) and report -1."""
    cfg, w, orc, om, picked, lists, tabs, refs = setup
    sup = sorted({p[0] for p in lists[0]})
    m = make_model(cfg, w, max_batch=3)
    ids, match = m.transcribe_batch(_mels(setup), constraint=lists[0], suppress_tokens=sup, **_kw(False))
    for b, (seed, mel, enc, first) in enumerate(picked):
        want = _ref_stream(orc, om, enc, PROMPT, tabs[(0, False)], suppress=sup)
        assert ids[b] == want[0] and want[3] == -1 and match[b] == -1, (ids[b], want[0])
        assert ids[b][NP:] == [0, EOT]
    m.close()


def test_refused_when_asked_for(hip, setup):
    """the library's own refusals behind the Python layer's: the pass's eot inside a phrase, a slot without a constrained pass, and
    the long-form and chunked entries while a table is set"""
    import ctypes as C
    from whisper_mojo_amd import _lib
    cfg, w, orc, om, picked, lists, tabs, refs = setup
    m = make_model(cfg, w, max_batch=3)
    L = _lib.lib()
    ip = C.POINTER(C.c_int32)
    out = np.zeros(3, np.int32)
    m.transcribe_batch(_mels(setup), **_kw(False))
    assert L.wm_transcribe_constraint_match(m._h, 0, out.ctypes.data_as(ip), 3) != 0
    ids, off = np.asarray([5, EOT], np.int32), np.asarray([0, 2], np.int32)
    assert L.wm_set_constraint(m._h, ids.ctypes.data_as(ip), off.ctypes.data_as(ip), 1, -1) == 0   # the eot is the pass's: checked there
    opts, keep = m._opts(PROMPT, EOT, 4, False, (), (), TS)
    toks, n = np.zeros((3, NP + 5), np.int32), np.zeros(3, np.int32)
    mels = np.ascontiguousarray(_mels(setup))
    assert L.wm_transcribe(m._h, mels.ctypes.data_as(C.c_void_p), 0, 3, C.byref(opts), toks.ctypes.data_as(ip), n.ctypes.data_as(ip)) != 0
    assert b"eot" in L.wm_last_error()
    assert L.wm_set_constraint(m._h, ids.ctypes.data_as(ip), off.ctypes.data_as(ip), 0, -1) != 0    # an empty list is not "off"
    ids[1] = 6
    assert L.wm_set_constraint(m._h, ids.ctypes.data_as(ip), off.ctypes.data_as(ip), 1, -1) == 0
    h = C.c_void_p()
    long_mel = np.zeros((1, cfg.n_mels, cfg.n_frames), np.float32)
    assert L.wm_transcribe_long(m._h, long_mel.ctypes.data_as(C.c_void_p), 0, 1, cfg.n_frames, None, C.byref(opts), C.byref(h)) != 0
    assert b"long-form" in L.wm_last_error()
    pcm = np.zeros((1, 16000), np.float32)
    ns, merged, mlen = np.array([16000], np.int32), np.zeros((1, 64), np.int32), np.zeros(1, np.int32)
    rc = L.wm_transcribe_chunked(m._h, pcm.ctypes.data_as(C.c_void_p), 0, ns.ctypes.data_as(ip), 1, 16000, 8000, 1000, 1000, C.byref(opts), None, 0,
                                 EOT, merged.ctypes.data_as(ip), mlen.ctypes.data_as(ip), 64, None, None, None)
    assert rc != 0 and b"chunked" in L.wm_last_error()
    assert L.wm_set_constraint(m._h, None, None, 0, -1) == 0
    m._ct_key = None
    m.close()
