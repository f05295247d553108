"""Per-utterance decoder prompts, CPU side: the host-only prompt builder (wm_op_long_prompt) against HF's own
_prepare_decoder_input_ids (tests/golden/long_prompt_rows.npz, tools/make_golden_prompts.py), its refusals, and the HF fixtures of
the GPU tests tied to the CPU oracle before any GPU is involved: the oracle decoding a single recording from a long prompt
(prompt_rows_micro_hf.npz), and the conditioned window loop — the oracle per window, wm_op_long_segments, wm_op_long_prompt —
against long_form_prompt_micro_hf.npz.  Exact equalities, no case left out.  The tiny fixtures are checked on the GPU only: the
oracle would take minutes per recording on them."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden
from test_long_form import restate_long_form

COND_TYPES = ("first-segment", "all-segments")


def _lib():
    import os
    from whisper_mojo_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L


def _segments(seq, count):
    out, first = [], 0
    for c in count.tolist():
        out.append(seq[first:first + c].tolist())
        first += c
    return out


def test_long_prompt_matches_hf_table():
    L = _lib()
    g = golden("long_prompt_rows")
    assert len(g["names"]) >= 30
    seen = set()
    for name in g["names"]:
        name = str(name)
        cond, ct, ctx, tb, prev_sot = (int(v) for v in g[name + "_opts"])
        pids = g[name + "_prompt_ids"].tolist() or None
        got = L.long_prompt(_segments(g[name + "_seq"], g[name + "_count"]), g[name + "_init"].tolist(), tb, ctx, prompt_ids=pids,
                            condition_on_prev_tokens=bool(cond), prompt_condition_type=COND_TYPES[ct], prev_sot_token=prev_sot)
        assert got == g[name + "_expect"].tolist(), name
        seen.add((ctx, cond, ct, pids is not None))
    assert {c[0] for c in seen} == {64, 448} and len(seen) >= 10  # both contexts, every combination of the options


def test_long_prompt_refuses_bad_arguments():
    L = _lib()
    ip = C.POINTER(C.c_int32)
    init = (C.c_int32 * 3)(1, 2, 3)
    seq = (C.c_int32 * 4)(941, 5, 6, 950)
    segs = (L.WmSegment * 1)(L.WmSegment(0, 4, 0.0, 0.0))
    out = (C.c_int32 * 64)()
    n = C.c_int32()
    pid = np.asarray([939, 7, 8], np.int32)

    def rc(seq=seq, segs=segs, n_segs=1, init=init, n_init=3, lo=None, tb=941, ctx=64, out=out, n_out=C.byref(n)):
        return L.lib().wm_op_long_prompt(seq, segs, n_segs, init, n_init, C.byref(lo) if lo is not None else None, tb, ctx, out, n_out)

    E_ARG = -1
    assert rc() == 0 and n.value == 3  # NULL options: the initial ids
    assert rc(lo=L.WmLongOpts(1, 939, None, 0, 0)) == 0 and list(out[:n.value]) == [939, 941, 5, 6, 950, 1, 2, 3]
    assert rc(init=None) == E_ARG and rc(n_init=0) == E_ARG and rc(out=None) == E_ARG and rc(n_out=None) == E_ARG
    assert rc(seq=None) == E_ARG and rc(segs=None) == E_ARG and rc(n_segs=-1) == E_ARG
    assert rc(tb=0) == E_ARG
    assert rc(lo=L.WmLongOpts(0, 939, pid.ctypes.data_as(ip), 3, 1)) == E_ARG  # all-segments without conditioning
    assert rc(lo=L.WmLongOpts(1, 939, pid.ctypes.data_as(ip), 3, 2)) == E_ARG  # unknown condition type
    assert rc(lo=L.WmLongOpts(1, 939, None, 3, 0)) == E_ARG                    # a count without ids
    assert rc(lo=L.WmLongOpts(1, -1, None, 0, 0)) == E_ARG                     # conditioning without <|startofprev|>
    long_pid = np.arange(4, 4 + 33, dtype=np.int32)
    assert rc(lo=L.WmLongOpts(1, 939, long_pid.ctypes.data_as(ip), 33, 1)) == E_ARG  # n_prompt_ids > n_text_ctx / 2
    bad = (L.WmSegment * 1)(L.WmSegment(-1, 4, 0.0, 0.0))
    assert rc(segs=bad) == E_ARG
    with pytest.raises(ValueError):
        L.long_prompt([], [1, 2, 3], 941, 64, prompt_condition_type="every-segment")
    assert rc() == 0 and n.value == 3  # still serves


@pytest.fixture(scope="module")
def micro_oracle(micro_cfg, micro_weights):
    from oracle import oracle
    return oracle.OracleModel(micro_cfg, micro_weights, gelu_mode=1)  # HF: erf GELU


def test_oracle_matches_hf_prompt_rows(micro_cfg, micro_oracle):
    """The existing oracle, decoding one recording from a prompt of 1 .. 31 ids, gives HF's ids: the fixture's rows are what a row
    of a ragged pass must give on its own."""
    from whisper_mojo_amd import synth
    g = golden("prompt_rows_micro_hf")
    lengths = set()
    for r in range(int(g["n_rows"])):
        prompt = g[f"r{r}_prompt"].tolist()
        ts = (int(g["timestamp_begin"]), int(g["no_ts"]), int(g["max_init"])) if int(g[f"r{r}_ts"]) else None
        got = micro_oracle.transcribe(synth.synth_mel(micro_cfg, int(g[f"r{r}_seed"])), prompt=prompt, eot=int(g["eos"]),
                                      max_loop=int(g["max_loop"]), pos_mode=1, timestamps=ts)
        assert got.tolist() == g[f"r{r}_ids"].tolist(), r
        assert len(prompt) + 1 + int(g["max_loop"]) <= micro_cfg.n_text_ctx
        lengths.add(len(prompt))
    assert lengths == {1, 4, 5, 16, 17, 31}


def restate_conditioned(decode_one, mels, n_frames, W, init, tb, eot, n_text_ctx, **popts):
    """The conditioned window loop: restate_long_form with a decoder that builds every window's prompt from the utterance's own
    segments so far (wm_op_long_prompt) — what wm_transcribe_long_ex does per row.  decode_one(window_mel, prompt) -> ids
    after the prompt (eot kept)."""
    from whisper_mojo_amd import _lib as L
    hist = [[] for _ in mels]
    longest = [0]

    def decode(items):
        out = []
        for b, s, snf in items:
            prompt = L.long_prompt(hist[b], init, tb, n_text_ctx, **popts)
            longest[0] = max(longest[0], len(prompt))
            win = np.zeros((mels[b].shape[0], W), np.float32)
            win[:, :snf] = mels[b][:, s:s + snf]
            ids = list(decode_one(win, prompt))
            out.append(ids)
            kept = ids[:-1] if ids and ids[-1] == eot else ids
            hist[b] += [kept[f:f + c] for f, c, _, _ in L.long_segments(kept, tb, s, snf)[0]]
        return out

    res, stalled = restate_long_form(decode, n_frames, W, tb, eot)
    return res, stalled, longest[0]


def long_prompt_case(g, case, cfg):
    from whisper_mojo_amd import synth
    lengths = [int(v) for v in g[case + "_lengths"]]
    mels = [synth.synth_long_mel(cfg, int(s), n) for s, n in zip(g[case + "_seeds"], lengths)]
    kw = dict(prompt=tuple(int(v) for v in g["prompt"]), eot=int(g["eos"]), max_loop=int(g[case + "_max_new_tokens"]) - 1,
              timestamps=(int(g["timestamp_begin"]), int(g["no_ts"]), 50))
    popts = dict(prompt_ids=g[case + "_prompt_ids"].tolist() or None, condition_on_prev_tokens=bool(int(g[case + "_cond"])),
                 prompt_condition_type=COND_TYPES[int(g[case + "_cond_type"])], prev_sot_token=int(g["prev_sot"]))
    return mels, lengths, kw, popts


def assert_matches_fixture(got, g, case, n):
    for b in range(n):
        assert got[b]["sequence"] == g[f"{case}_u{b}_sequence"].tolist(), (case, b)
        assert [len(s["tokens"]) for s in got[b]["segments"]] == g[f"{case}_u{b}_count"].tolist(), (case, b)
        # float64, bit for bit
        assert [s["start"] for s in got[b]["segments"]] == g[f"{case}_u{b}_start"].tolist(), (case, b)
        assert [s["end"] for s in got[b]["segments"]] == g[f"{case}_u{b}_end"].tolist(), (case, b)


def test_conditioned_window_loop_matches_hf_micro(micro_cfg, micro_oracle):
    g = golden("long_form_prompt_micro_hf")
    cut = micro_cfg.n_text_ctx // 2 - 1
    cases = [str(c) for c in g["cases"]]
    assert {"cond", "first_segment", "all_segments", "prompt_no_cond", "long_history", "max_new"} <= set(cases)
    full_history = False
    for case in cases:
        mels, lengths, kw, popts = long_prompt_case(g, case, micro_cfg)

        def decode_one(win, prompt):
            ids = micro_oracle.transcribe(win, prompt=prompt, eot=kw["eot"], max_loop=kw["max_loop"], pos_mode=1, timestamps=kw["timestamps"])
            return ids[len(prompt):].tolist()

        got, _stalled, longest = restate_conditioned(decode_one, mels, lengths, micro_cfg.n_frames, list(kw["prompt"]), kw["timestamps"][0],
                                                     kw["eot"], micro_cfg.n_text_ctx, **popts)
        assert_matches_fixture(got, g, case, len(lengths))
        assert longest + 1 + kw["max_loop"] <= micro_cfg.n_text_ctx
        full_history |= popts["condition_on_prev_tokens"] and longest >= 1 + cut + len(kw["prompt"])
    assert full_history  # some window carried the whole cut_off_length of history
