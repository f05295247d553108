"""Sequential long-form transcription, CPU side: the host-only segment splitter (wm_op_long_segments) against HF's own
_retrieve_segment (tests/golden/long_form_segments.npz, tools/make_golden_long_form.py), the zero-advance rule of the window
loop, and the self-consistency of the long-form fixtures.  restate_long_form is the window loop in numpy over any per-window
decoder; the GPU tests compose it with transcribe_batch."""
import numpy as np
import pytest

from conftest import golden


def _lib():
    import os
    from whisper_mojo_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L


def restate_long_form(decode, n_frames, W, timestamp_begin, eot):
    """The window loop of wm_transcribe_long.  decode(items) -> one list of ids (prompt excluded, eot kept when hit) per
    (utterance, seek, seek_num_frames) item.  Returns (results shaped like Whisper.transcribe_long_form, stalled windows)."""
    from whisper_mojo_amd import _lib as L
    B = len(n_frames)
    seek = [0] * B
    out = [{"sequence": [], "segments": []} for _ in range(B)]
    stalled = 0
    while True:
        items = [(b, seek[b], min(n_frames[b] - seek[b], W)) for b in range(B) if seek[b] < n_frames[b]]
        if not items:
            return out, stalled
        for (b, s, snf), ids in zip(items, decode(items)):
            ids = list(ids)
            if ids and ids[-1] == eot:
                ids = ids[:-1]
            segs, adv = L.long_segments(ids, timestamp_begin, s, snf)
            if adv == 0:  # the documented deviation: advance by the window instead of decoding it again
                adv, stalled = snf, stalled + 1
            for first, count, start, end in segs:
                toks = ids[first:first + count]
                out[b]["sequence"] += toks
                out[b]["segments"].append({"start": start, "end": end, "tokens": toks})
            seek[b] += adv


def test_segments_match_hf_table():
    L = _lib()
    g = golden("long_form_segments")
    tb = int(g["timestamp_begin"])
    for name in g["names"]:
        name = str(name)
        segs, adv = L.long_segments(g[name + "_ids"], tb, int(g[name + "_seek"]), int(g[name + "_snf"]))
        assert adv == int(g[name + "_advance"]), name
        assert [s[0] for s in segs] == g[name + "_first"].tolist(), name
        assert [s[1] for s in segs] == g[name + "_count"].tolist(), name
        # float64 bit for bit
        assert np.array_equal(np.asarray([s[2] for s in segs], np.float64).view(np.int64), g[name + "_start"].view(np.int64)), name
        assert np.array_equal(np.asarray([s[3] for s in segs], np.float64).view(np.int64), g[name + "_end"].view(np.int64)), name


def test_zero_advance_follows_documented_rule():
    """HF returns advance 0 for <|0.00|><|0.00|> (and decodes the same window forever); the loop advances by the window,
    keeps its segments once and counts it."""
    L = _lib()
    tb = 941
    segs, adv = L.long_segments([tb, tb], tb, 200, 200)
    assert adv == 0 and len(segs) == 1 and segs[0][:2] == (0, 2)
    calls = []

    def decode(items):
        calls.append(items)
        return [[tb, tb, 900] if s == 0 else [tb, 5, 6, tb + 10, 900] for _, s, _ in items]

    out, stalled = restate_long_form(decode, [350], 200, tb, 900)
    assert stalled == 1
    assert [c[0][1:] for c in calls] == [(0, 200), (200, 150)]
    assert out[0]["sequence"] == [tb, tb, tb, 5, 6, tb + 10]
    assert [(s["start"], s["end"]) for s in out[0]["segments"]] == [(0.0, 0.0), (2.0, 2.0 + 10 * 0.02)]


def test_op_refuses_bad_arguments():
    import ctypes as C
    L = _lib()
    segs = (L.WmSegment * 2)()
    n, adv = C.c_int32(), C.c_int32()
    ids = (C.c_int32 * 2)(1, 2)
    assert L.lib().wm_op_long_segments(ids, 2, 0, 0, 100, segs, C.byref(n), C.byref(adv)) == -1  # no timestamp rules
    assert L.lib().wm_op_long_segments(ids, 2, 941, -1, 100, segs, C.byref(n), C.byref(adv)) == -1
    assert L.lib().wm_op_long_segments(None, 2, 941, 0, 100, segs, C.byref(n), C.byref(adv)) == -1


@pytest.mark.parametrize("name", ["micro", "tiny"])
def test_long_form_fixture_self_consistent(name):
    from whisper_mojo_amd import WhisperConfig
    cfg = WhisperConfig.micro() if name == "micro" else WhisperConfig.tiny()
    g = golden(f"long_form_{name}_hf")
    tb = int(g["timestamp_begin"])
    assert tb == int(g["no_ts"]) + 1 and int(g["eos"]) < tb
    short_in_long = False
    for case in g["cases"]:
        case = str(case)
        lengths = g[case + "_lengths"]
        assert len(g[case + "_seeds"]) == len(lengths)
        assert len(g["prompt"]) + int(g[case + "_max_new_tokens"]) <= cfg.n_text_ctx
        short_in_long |= bool(lengths.min() <= cfg.n_frames < lengths.max())
        for b in range(len(lengths)):
            seq, cnt = g[f"{case}_u{b}_sequence"], g[f"{case}_u{b}_count"]
            start, end = g[f"{case}_u{b}_start"], g[f"{case}_u{b}_end"]
            assert cnt.sum() == len(seq) and len(cnt) == len(start) == len(end) >= 1
            assert start[0] >= 0.0 and (seq != int(g["eos"])).all()
            assert end[-1] <= lengths[b] * 0.01 + 30.0
    assert short_in_long


def test_long_logmel_fixture_mask_rule():
    g = golden("long_form_logmel")
    n = g["n_samples"]
    F = int(n.max()) // 160
    assert g["n_frames"].tolist() == [min(-(-int(v) // 160), F) for v in n]
    assert g["mel_cols"].shape == (len(n), 80, len(g["cols"])) and g["cols"].max() < F
    assert (g["mel_cols"].max(axis=(1, 2)) <= g["mel_max"]).all() and (g["mel_cols"].min(axis=(1, 2)) >= g["mel_max"] - 2.0 - 1e-5).all()
