"""Replay or recapture (-m gpu): one state runs different kinds of pass one after another, and every pass must give what the same
request gives on a fresh model that has run nothing else — bit for bit, ids and whatever else the pass produces.  A captured loop
step that is replayed for a pass it was not captured for (another eot, stop rule, timestamp rules, log-probs, key windows,
alignment capture, chip sharing) shows up here as different ids, log-probs or times.

Micro config, synthetic weights, B = 3, max_loop = 12 (the loop is enqueued whole, so every pass runs max_loop graph replays);
every call goes through ctypes with its own buffers.  Nine fresh models in all, one at a time."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, MAX_LOOP = 3, 12
PROMPT = (1, 2, 3, 4)
STRIDE = len(PROMPT) + 1 + MAX_LOOP
ROW_PROMPTS = ((1, 2, 3, 4), (2, 3, 4), (3, 4))
TS_BEGIN, MAX_INIT = 900, 10
HEADS = {"tt": ((0, 0), (1, 1)), "tt_other_heads": ((0, 1), (1, 0)), "align": ((0, 0), (1, 1))}
# the align pass: rows of 22, 10 and 15 ids behind a 4-id context, so its longest row has 17 timed ids — more than MAX_LOOP, which
# re-sizes the capture buffer the timestamp pass before it had captured into
ALIGN_STRIDE, ALIGN_LEN, ALIGN_CTX = 24, (22, 10, 15), (4, 4, 4)

FP, IP = C.POINTER(C.c_float), C.POINTER(C.c_int32)


def f(a):
    return a.ctypes.data_as(FP)


def i(a):
    return a.ctypes.data_as(IP)


class Runner:
    """One model and the raw calls.  run(kind, eot) is the synchronous call, submit / wait the pipelined pair; a result is a tuple
    of byte strings (counts, ids, then log-probs or times), so equality is bitwise."""

    def __init__(self, cfg, weights):
        from whisper_mojo_amd import _lib, synth
        from whisper_mojo_amd.loader import WeightLoader
        from whisper_mojo_amd.whisper import Whisper
        self.lib, self.L = _lib, _lib.lib()
        self.model = Whisper(cfg, max_batch=B)
        self.model.load(WeightLoader.from_array(weights))
        self.h = self.model._h
        self.mel = np.ascontiguousarray(synth.synth_mels(cfg, 0, B), np.float32)
        self.prompt = np.asarray(PROMPT, np.int32)
        self.rows = np.zeros((B, 4), np.int32)
        for b, r in enumerate(ROW_PROMPTS):
            self.rows[b, :len(r)] = r
        self.row_len = np.asarray([len(r) for r in ROW_PROMPTS], np.int32)
        self.ids = np.zeros((B, ALIGN_STRIDE), np.int32)
        for b, n in enumerate(ALIGN_LEN):
            self.ids[b, :n] = [(7 * k + 3 * b + 5) % 800 + 1 for k in range(n)]
            self.ids[b, :len(PROMPT)] = PROMPT
        self.ids_len, self.ctx = np.asarray(ALIGN_LEN, np.int32), np.asarray(ALIGN_CTX, np.int32)

    def close(self):
        self.model.close()

    def opts(self, kind, eot):
        """(a) plain: no stop; (b) eot: rows stop at `eot`; (c) ignore_eot: ... but run on; (d) rules and later: the timestamp rules
        on top of (c)."""
        rules = kind not in ("plain", "eot", "ignore_eot")
        return self.lib.WmDecodeOpts(i(self.prompt), len(PROMPT), -1 if kind == "plain" else eot, MAX_LOOP, self.model.pos_mode,
                                     0 if kind in ("plain", "eot") else 1, None, 0, None, 0, TS_BEGIN if rules else 0, -1,
                                     MAX_INIT if rules else -1)

    def _bufs(self):
        self.toks, self.n = np.zeros((B, STRIDE), np.int32), np.zeros(B, np.int32)
        self.tab, self.avg = np.zeros((B, STRIDE), np.float32), np.zeros(B, np.float32)
        self.times = np.zeros((B, ALIGN_STRIDE), np.float32)

    def run(self, kind, eot):
        L, o = self.L, C.byref(self.opts(kind, eot))
        a, t = (self.h, self.mel.ctypes.data_as(C.c_void_p), 0, B), None
        self._bufs()
        t = (i(self.toks), i(self.n))
        if kind in HEADS:
            self.model.set_alignment_heads(HEADS[kind])
        if kind == "lp":
            rc, extra = L.wm_transcribe_lp(*a, o, None, None, 0, *t, f(self.tab), f(self.avg)), (self.tab, self.avg)
        elif kind == "rows":
            rc, extra = L.wm_transcribe_rows(*a, o, i(self.rows), i(self.row_len), 4, *t), ()
        elif kind in ("tt", "tt_other_heads"):
            rc, extra = L.wm_transcribe_tt(*a, o, None, *t, f(self.tab)), (self.tab,)
        elif kind == "align":
            rc = L.wm_align(*a, self.model.pos_mode, i(self.ids), i(self.ids_len), ALIGN_STRIDE, i(self.ctx), None, f(self.times), None, None, None)
            extra = (self.times,)
        else:
            rc, extra = L.wm_transcribe(*a, o, *t), ()
        assert rc == 0, (kind, L.wm_last_error().decode())
        return self._result(extra)

    def _result(self, extra):
        """What the caller may read, as bytes: the counts, per row the ids and table entries below the row's count (an align
        pass: below its ids_len), per-row scalars whole."""
        n = self.ids_len if any(x is self.times for x in extra) else self.n
        parts = [self.n.tobytes()]
        for x in (self.toks,) + tuple(extra):
            parts.append(b"".join(x[b, :n[b]].tobytes() for b in range(B)) if x.ndim == 2 else x.tobytes())
        return tuple(parts)

    def submit_wait(self, kind, eot, slot):
        L, o = self.L, C.byref(self.opts(kind, eot))
        a = (self.h, slot, self.mel.ctypes.data_as(C.c_void_p), 0, B)
        self._bufs()
        if kind == "tt":
            self.model.set_alignment_heads(HEADS[kind])
            assert L.wm_transcribe_submit_tt(*a, o, None) == 0, L.wm_last_error().decode()
            rc, extra = L.wm_transcribe_wait_tt(self.h, slot, i(self.toks), i(self.n), f(self.tab)), (self.tab,)
        else:
            assert L.wm_transcribe_submit(*a, o) == 0, L.wm_last_error().decode()
            rc, extra = L.wm_transcribe_wait(self.h, slot, i(self.toks), i(self.n)), ()
        assert rc == 0, (kind, slot, L.wm_last_error().decode())
        return self._result(extra)


def lengths(result):
    return np.frombuffer(result[0], np.int32)


@pytest.fixture(scope="module")
def fresh(micro_cfg, micro_weights):
    """kind -> what the request gives on a model that has run nothing else, and the eot id of passes (b) and later: an id below
    TS_BEGIN that pass (a) emits in mid-transcript, so a row of (b) stops early."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")

    def one(kind, eot):
        r = Runner(micro_cfg, micro_weights)
        try:
            return r.run(kind, eot)
        finally:
            r.close()

    out = {"plain": one("plain", -1)}
    assert (lengths(out["plain"]) == STRIDE).all()  # (a) never stops: every row is full
    ids = np.frombuffer(out["plain"][1], np.int32).reshape(B, STRIDE)
    mid = [int(t) for t in ids[:, len(PROMPT) + 2:len(PROMPT) + 8].ravel() if 0 <= t < TS_BEGIN]
    assert mid, ids
    eot = mid[0]
    for kind in ("eot", "ignore_eot", "rules", "lp", "rows", "tt", "tt_other_heads", "align"):
        out[kind] = one(kind, eot)
    return out, eot


def test_passes_of_every_kind_on_one_state(micro_cfg, micro_weights, fresh):
    """(a) plain, (b) another eot, (c) ignore_eot, (d) timestamp rules, (e) log-probs, (f) per-row prompts, (g) token timestamps,
    (g') the same with other alignment heads, (h) an align pass that re-sizes the capture buffer, (i) = (g), (j) = (a), all
    synchronous on one model: each equals the fresh model's result."""
    want, eot = fresh
    assert (lengths(want["eot"]) < lengths(want["plain"])).any(), "the eot id must stop a row early"
    assert want["tt"][2] != want["tt_other_heads"][2], "the two head sets must give different times"
    r = Runner(micro_cfg, micro_weights)
    try:
        for step, kind in zip("abcdefgGhij", ("plain", "eot", "ignore_eot", "rules", "lp", "rows", "tt", "tt_other_heads", "align", "tt", "plain")):
            assert r.run(kind, eot) == want[kind], f"pass ({step}) {kind}"
    finally:
        r.close()


def test_pipelined_and_synchronous_passes_take_turns(micro_cfg, micro_weights, fresh):
    """A pipelined pass shares the chip, a synchronous one does not: (a) on slot 1, (a) synchronously (slot 0's state), then on
    slot 1 (a), a timestamp pass and (a) again — every result equals the fresh model's."""
    want, eot = fresh
    r = Runner(micro_cfg, micro_weights)
    try:
        assert r.submit_wait("plain", eot, 1) == want["plain"]
        assert r.run("plain", eot) == want["plain"]
        assert r.submit_wait("plain", eot, 1) == want["plain"]
        assert r.submit_wait("tt", eot, 1) == want["tt"]
        assert r.submit_wait("plain", eot, 1) == want["plain"]
        assert r.run("plain", eot) == want["plain"]
    finally:
        r.close()
