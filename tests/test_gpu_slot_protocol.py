"""The slot protocol of the C ABI (-m gpu): which wait collects which submit, what a refused wait or submit leaves behind, which
submits a coalesce = 2 model pairs, and when wm_alignment_weights still serves a slot.  Micro config, synthetic weights, B = 2,
max_loop = 4, two alignment heads, three languages; every call goes through ctypes with its own buffers."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E_STATE = -5
B, MAX_LOOP, STRIDE = 2, 4, 9  # STRIDE = n_prompt + 1 + max_loop = the width of every id / time / log-prob table below
PROMPT = (1, 2, 3, 4)
ROW_PROMPTS = ((1, 2, 3, 4), (2, 3, 4))
LANGS = (10, 11, 12)
NS_TOKEN = 5
SCORE_IDS = ((1, 2, 3, 4, 7, 8, 9), (1, 2, 3, 4, 7, 8))
SCORE_CTX = (4, 4)
HEADS = ((0, 0), (1, 1))

FP, IP = C.POINTER(C.c_float), C.POINTER(C.c_int32)


def f(a):
    return a.ctypes.data_as(FP)


def i(a):
    return a.ctypes.data_as(IP)


SCORE_MSG = "this slot holds a score pass (collect it with wm_score_wait)"
ALIGN_MSG = "this slot holds an align pass (collect it with wm_align_wait)"
TRANS_MSG = "this slot holds a transcribe pass (collect it with wm_transcribe_wait)"
ALIGN_LP_MSG = "this slot's align pass was submitted without log-probabilities"
PENDING_MSG = "this slot still holds a pass that was not waited for"
NEED_MSG = {  # in the order the waits check them
    "lang": "this slot's pass was submitted without language detection (wm_transcribe_submit_lang)",
    "ns": "this slot's pass was submitted without the no-speech probe (wm_transcribe_submit_lp_ns)",
    "lp": "this slot's pass was submitted without log-probabilities (wm_transcribe_submit_lp)",
    "tt": "this slot's pass was submitted without token timestamps (wm_transcribe_submit_tt)",
}
# submit -> (kind of pass, what it computes, the wait that collects all of it)
SUBMITS = {
    "plain": ("transcribe", set(), "wait"),
    "tt": ("transcribe", {"tt"}, "wait_tt"),
    "rows": ("transcribe", set(), "wait"),
    "lp": ("transcribe", {"lp"}, "wait_lp"),
    "lp_ns": ("transcribe", {"lp", "ns"}, "wait_lp_ns"),
    "lang": ("transcribe", {"lang"}, "wait_lang"),
    "lang_lp": ("transcribe", {"lang", "lp"}, "wait_lang_lp"),
    "score": ("score", set(), "score_wait"),
    "align": ("align", set(), "align_wait"),
    "align_lp": ("align", {"lp"}, "align_wait_lp"),
}
# wait -> (kind of pass it collects, what it asks for)
WAITS = {
    "wait": ("transcribe", set()),
    "wait_tt": ("transcribe", {"tt"}),
    "wait_lp": ("transcribe", {"lp"}),
    "wait_lp_ns": ("transcribe", {"lp", "ns"}),
    "wait_lang": ("transcribe", {"lang"}),
    "wait_lang_lp": ("transcribe", {"lang", "lp"}),
    "wait_device": ("transcribe", set()),
    "score_wait": ("score", set()),
    "align_wait": ("align", set()),
    "align_wait_lp": ("align", {"lp"}),
}


def refusal(submit, wait):
    """The message of the WM_E_STATE a wait answers a slot holding this submit with; None: it collects the pass."""
    kind, has, _ = SUBMITS[submit]
    wkind, asks = WAITS[wait]
    if kind != wkind:
        return {"score": SCORE_MSG, "align": ALIGN_MSG, "transcribe": TRANS_MSG}[kind]
    if kind == "align":
        return ALIGN_LP_MSG if asks - has else None
    for what in ("lang", "ns", "lp", "tt"):
        if what in asks and what not in has:
            return NEED_MSG[what]
    return None


class Proto:
    """One model and the raw calls: submit(kind, slot, mel) / wait(kind, slot) / sync(kind, mel).  A wait or sync call returns
    (rc, result): the id lists of a transcribe pass, the log-prob table of a score pass, the time table of an align pass."""

    def __init__(self, cfg, weights, coalesce=0):
        from whisper_mojo_amd import _lib
        from whisper_mojo_amd.loader import WeightLoader
        from whisper_mojo_amd.whisper import Whisper
        self.L = _lib.lib()
        self.model = Whisper(cfg, max_batch=B, coalesce=coalesce)
        self.model.load(WeightLoader.from_array(weights))
        self.model.set_alignment_heads(HEADS)
        self.h = self.model._h
        self.prompt = np.asarray(PROMPT, np.int32)
        self.opts = _lib.WmDecodeOpts(i(self.prompt), len(PROMPT), -1, MAX_LOOP, self.model.pos_mode, 0, None, 0, None, 0, 0, -1, -1)
        self.rows = np.zeros((B, 4), np.int32)
        for b, r in enumerate(ROW_PROMPTS):
            self.rows[b, :len(r)] = r
        self.row_len = np.asarray([len(r) for r in ROW_PROMPTS], np.int32)
        self.langs = np.asarray(LANGS, np.int32)
        self.ids = np.zeros((B, STRIDE), np.int32)
        for b, r in enumerate(SCORE_IDS):
            self.ids[b, :len(r)] = r
        self.ids_len = np.asarray([len(r) for r in SCORE_IDS], np.int32)
        self.ctx = np.asarray(SCORE_CTX, np.int32)
        self.toks, self.n = np.zeros((B, STRIDE), np.int32), np.zeros(B, np.int32)
        self.times, self.lps = np.zeros((B, STRIDE), np.float32), np.zeros((B, STRIDE), np.float32)
        self.top = np.zeros((B, STRIDE), np.int32)
        self.avg, self.sm, self.nsp = np.zeros(B, np.float32), np.zeros(B, np.float32), np.zeros(B, np.float32)
        self.lang_out, self.lang_probs = np.zeros(B, np.int32), np.zeros((B, len(LANGS)), np.float32)

    def close(self):
        self.model.close()

    def error(self):
        return self.L.wm_last_error().decode()

    def _ids(self):
        return [self.toks[b, :self.n[b]].tolist() for b in range(B)]

    def submit(self, kind, slot, mel):
        L, h, o = self.L, self.h, C.byref(self.opts)
        a = (h, slot, mel.ctypes.data_as(C.c_void_p), 0, B)
        rows = (i(self.rows), i(self.row_len), 4)
        score = (self.model.pos_mode, i(self.ids), i(self.ids_len), STRIDE, i(self.ctx))
        return {
            "plain": lambda: L.wm_transcribe_submit(*a, o),
            "tt": lambda: L.wm_transcribe_submit_tt(*a, o, None),
            "rows": lambda: L.wm_transcribe_submit_rows(*a, o, *rows),
            "lp": lambda: L.wm_transcribe_submit_lp(*a, o, None, None, 0),
            "lp_ns": lambda: L.wm_transcribe_submit_lp_ns(*a, o, None, None, 0, NS_TOKEN, len(PROMPT)),
            "lang": lambda: L.wm_transcribe_submit_lang(*a, o, None, None, 0, -1, len(PROMPT), i(self.langs), len(LANGS), 0),
            "lang_lp": lambda: L.wm_transcribe_submit_lang(*a, o, None, None, 0, -1, len(PROMPT), i(self.langs), len(LANGS), 1),
            "score": lambda: L.wm_score_submit(*a, *score),
            "align": lambda: L.wm_align_submit(*a, *score, None, 0),
            "align_lp": lambda: L.wm_align_submit(*a, *score, None, 1),
        }[kind]()

    def sync(self, kind, mel):
        L, h, o = self.L, self.h, C.byref(self.opts)
        a = (h, mel.ctypes.data_as(C.c_void_p), 0, B)
        t = (i(self.toks), i(self.n))
        rows = (i(self.rows), i(self.row_len), 4)
        lang = (None, None, 0, -1, len(PROMPT), i(self.langs), len(LANGS))
        score = (self.model.pos_mode, i(self.ids), i(self.ids_len), STRIDE, i(self.ctx))
        rc = {
            "plain": lambda: L.wm_transcribe(*a, o, *t),
            "tt": lambda: L.wm_transcribe_tt(*a, o, None, *t, f(self.times)),
            "rows": lambda: L.wm_transcribe_rows(*a, o, *rows, *t),
            "lp": lambda: L.wm_transcribe_lp(*a, o, None, None, 0, *t, f(self.lps), f(self.avg)),
            "lp_ns": lambda: L.wm_transcribe_lp_ns(*a, o, None, None, 0, NS_TOKEN, len(PROMPT), *t, f(self.lps), f(self.avg), f(self.nsp)),
            "lang": lambda: L.wm_transcribe_lang(*a, o, *lang, *t, None, None, None, i(self.lang_out), f(self.lang_probs)),
            "lang_lp": lambda: L.wm_transcribe_lang(*a, o, *lang, *t, f(self.lps), f(self.avg), None, i(self.lang_out), f(self.lang_probs)),
            "score": lambda: L.wm_score(*a, *score, f(self.lps), i(self.top), f(self.sm), f(self.avg)),
            "align": lambda: L.wm_align(*a, *score, None, f(self.times), None, None, None),
            "align_lp": lambda: L.wm_align(*a, *score, None, f(self.times), f(self.lps), f(self.sm), f(self.avg)),
        }[kind]()
        return rc, self._result(SUBMITS[kind][0])

    def _result(self, kind):
        return self.lps.copy() if kind == "score" else self.times.copy() if kind == "align" else self._ids()

    def wait(self, kind, slot):
        L, a = self.L, (self.h, slot)
        t = (i(self.toks), i(self.n))
        if kind == "wait_device":
            import torch
            packed = torch.zeros((B, 1 + STRIDE), dtype=torch.int32, device="cuda")
            rc = L.wm_transcribe_wait_device(*a, C.c_void_p(packed.data_ptr()), B, STRIDE)
            p = packed.cpu().numpy()
            return rc, [p[b, 1:1 + p[b, 0]].tolist() for b in range(B)]
        rc = {
            "wait": lambda: L.wm_transcribe_wait(*a, *t),
            "wait_tt": lambda: L.wm_transcribe_wait_tt(*a, *t, f(self.times)),
            "wait_lp": lambda: L.wm_transcribe_wait_lp(*a, *t, f(self.lps), f(self.avg)),
            "wait_lp_ns": lambda: L.wm_transcribe_wait_lp_ns(*a, *t, f(self.lps), f(self.avg), f(self.nsp)),
            "wait_lang": lambda: L.wm_transcribe_wait_lang(*a, *t, None, None, None, i(self.lang_out), f(self.lang_probs)),
            "wait_lang_lp": lambda: L.wm_transcribe_wait_lang(*a, *t, f(self.lps), f(self.avg), None, i(self.lang_out), f(self.lang_probs)),
            "score_wait": lambda: L.wm_score_wait(*a, f(self.lps), i(self.top), f(self.sm), f(self.avg)),
            "align_wait": lambda: L.wm_align_wait(*a, f(self.times), None, None, None),
            "align_wait_lp": lambda: L.wm_align_wait(*a, f(self.times), f(self.lps), f(self.sm), f(self.avg)),
        }[kind]()
        return rc, self._result(WAITS[kind][0])


def same(a, b):
    return np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b


@pytest.fixture(scope="module")
def proto(micro_cfg, micro_weights):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    p = Proto(micro_cfg, micro_weights)
    yield p
    p.close()


@pytest.fixture(scope="module")
def mels(micro_cfg):
    from whisper_mojo_amd import synth
    return [np.ascontiguousarray(synth.synth_mels(micro_cfg, 10 * k, B), np.float32) for k in range(2)]


@pytest.fixture(scope="module")
def want(proto, mels):
    """(submit kind, mel index) -> the synchronous call's result, computed once"""
    out = {}
    for kind in SUBMITS:
        for k, mel in enumerate(mels):
            rc, out[kind, k] = proto.sync(kind, mel)
            assert rc == 0, (kind, proto.error())
    return out


@pytest.mark.parametrize("submit", list(SUBMITS))
def test_submit_kind_times_wait_kind(proto, mels, want, submit):
    """Every wait on a slot holding every kind of pass: a refusal is WM_E_STATE with its exact text and leaves the pass pending —
    the pass's own wait then delivers the synchronous call's result; a wait that asks for no more than the pass computed collects
    it."""
    slot, own = 1, SUBMITS[submit][2]
    for wait in WAITS:
        assert proto.submit(submit, slot, mels[0]) == 0, (wait, proto.error())
        msg = refusal(submit, wait)
        rc, got = proto.wait(wait, slot)
        if msg is None:
            assert rc == 0, (wait, proto.error())
            assert same(got, want[submit, 0]), wait
            continue
        assert rc == E_STATE and proto.error() == msg, (wait, rc, proto.error())
        rc, got = proto.wait(own, slot)
        assert rc == 0, (wait, proto.error())
        assert same(got, want[submit, 0]), wait
    rc, _ = proto.wait(own, slot)  # nothing is left on the slot
    assert rc == E_STATE and proto.error() == "nothing was submitted on this slot"


@pytest.mark.parametrize("slot", [0, 3])
def test_second_submit_on_a_pending_slot_is_refused(proto, mels, want, slot):
    """A submit of any kind on a slot whose pass was not waited for returns WM_E_STATE; the first pass is collected intact."""
    for first, second in [("plain", k) for k in SUBMITS] + [(k, "plain") for k in SUBMITS if k != "plain"]:
        assert proto.submit(first, slot, mels[0]) == 0, (first, proto.error())
        assert proto.submit(second, slot, mels[1]) == E_STATE and proto.error() == PENDING_MSG, (first, second, proto.error())
        rc, got = proto.wait(SUBMITS[first][2], slot)
        assert rc == 0 and same(got, want[first, 0]), (first, second, proto.error())


def test_coalesce_pairs_matching_submits_only(proto, mels, want, micro_cfg, micro_weights):
    """coalesce = 2: two matching submits share one pass and each wait returns its own batch's ids; a plain submit followed by an
    _lp submit does not pair, and both return the uncoalesced ids."""
    pair = Proto(micro_cfg, micro_weights, coalesce=2)
    try:
        for a, b in (("plain", "plain"), ("lp", "lp"), ("plain", "lp"), ("lp", "plain")):
            assert pair.submit(a, 0, mels[0]) == 0 and pair.submit(b, 1, mels[1]) == 0, (a, b, pair.error())
            rc, got = pair.wait(SUBMITS[b][2], 1)
            assert rc == 0 and got == want[b, 1], (a, b, pair.error())
            rc, got = pair.wait(SUBMITS[a][2], 0)
            assert rc == 0 and got == want[a, 0], (a, b, pair.error())
    finally:
        pair.close()


def test_alignment_weights_follow_the_slots_last_pass(proto, mels, want):
    """wm_alignment_weights serves a slot only while its last collected pass is a timestamp pass: a later pass without timestamps on
    the same state (wm_transcribe_pcm on slot 0, wm_transcribe_submit / wm_transcribe_wait_device on slot 1) ends that."""
    L, h = proto.L, proto.h
    W = np.zeros((B, len(HEADS), MAX_LOOP, proto.model.config.n_audio_ctx), np.float32)
    no_pass = "no completed timestamp pass on this slot (or its state has run another pass since)"
    rc, got = proto.sync("tt", mels[0])
    assert rc == 0 and got == want["tt", 0]
    assert L.wm_alignment_weights(h, 0, f(W)) == 0 and W.any()
    pcm = np.zeros((B, 1600), np.float32)
    pcm[:] = np.sin(np.arange(1600) * 0.05)
    n_samples = np.full(B, 1600, np.int32)
    assert L.wm_transcribe_pcm(h, f(pcm), i(n_samples), B, 1600, C.byref(proto.opts), i(proto.toks), i(proto.n)) == 0, proto.error()
    assert L.wm_alignment_weights(h, 0, f(W)) == E_STATE and proto.error() == no_pass
    # slot 1: a timestamp pass, then a plain pass collected on the device
    assert proto.submit("tt", 1, mels[0]) == 0
    rc, got = proto.wait("wait_tt", 1)
    assert rc == 0 and got == want["tt", 0]
    assert L.wm_alignment_weights(h, 1, f(W)) == 0 and W.any()
    assert proto.submit("plain", 1, mels[1]) == 0
    rc, got = proto.wait("wait_device", 1)
    assert rc == 0 and got == want["plain", 1]
    assert L.wm_alignment_weights(h, 1, f(W)) == E_STATE and proto.error() == no_pass
