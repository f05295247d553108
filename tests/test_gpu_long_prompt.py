"""GPU: long-form transcription with condition_on_prev_tokens / prompt_ids (wm_transcribe_long_ex) against HF generate's
long-form path with the same options (tests/golden/long_form_prompt_*_hf.npz, every recording run alone, tools/make_golden_prompts.py):
sequence, segment counts, start and end bit for bit, every case and utterance; schedule independence with conditioning on; and zero
options == wm_transcribe_long."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden
from test_gpu_long_form import assert_same, make_model
from test_long_prompt import assert_matches_fixture, long_prompt_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from whisper_mojo_amd import _lib
    _lib.lib()
    return True


@pytest.mark.parametrize("name", ["micro", "tiny"])
def test_matches_hf_long_form_prompts_fp32(hip, name, micro_cfg, micro_weights, tiny_cfg, tiny_weights):
    cfg, w = (micro_cfg, micro_weights) if name == "micro" else (tiny_cfg, tiny_weights)
    g = golden(f"long_form_prompt_{name}_hf")
    m = make_model(cfg, w, max_batch=4)
    cases = [str(c) for c in g["cases"]]
    assert {"cond", "first_segment", "all_segments", "prompt_no_cond", "long_history", "max_new"} <= set(cases)
    for case in cases:
        mels, lengths, kw, popts = long_prompt_case(g, case, cfg)
        got, st = m.transcribe_long_form(mels, return_stats=True, **kw, **popts)
        assert_matches_fixture(got, g, case, len(lengths))
        assert st["row_passes"] >= 1 and st["longest_prompt"] + 1 + kw["max_loop"] <= cfg.n_text_ctx
        if case == "long_history":
            # the scheduler itself built, cut and prefilled a full-length prompt: <|startofprev|> + cut_off_length ids + the initial ids
            # (tiny: 1 + 223 + 3 = 227 ids, 15 prefill chunks); the fixture alone shows the history was there to cut
            cut = cfg.n_text_ctx // 2 - 1
            assert st["longest_prompt"] == 1 + cut + len(kw["prompt"]), (name, st)
            assert max(len(g[f"{case}_u{b}_sequence"]) - len(g[f"{case}_u{b}_count"]) - kw["max_loop"] - 1 for b in range(len(lengths))) > cut
    if name == "tiny":
        # the long recording in one batch with the three of the `cond` case (same options): passes then mix a 227-id row with 3-id and
        # mid-length rows, and every recording still gives its own fixture result
        ml, ll, kw, popts = long_prompt_case(g, "long_history", cfg)
        mc, lc, kwc, poptsc = long_prompt_case(g, "cond", cfg)
        assert kw == kwc and popts == poptsc
        got, st = m.transcribe_long_form(mc[:1] + ml + mc[1:], return_stats=True, **kw, **popts)
        assert st["longest_prompt"] == 1 + (cfg.n_text_ctx // 2 - 1) + len(kw["prompt"])
        assert_matches_fixture([got[1]], g, "long_history", 1)
        assert_matches_fixture([got[0]] + got[2:], g, "cond", len(lc))
    m.close()


def test_scheduling_invariance_with_conditioning(hip, tiny_cfg, tiny_weights):
    """5 utterances on max_batch = 2 = each alone = max_batch = 8, bitwise, with every window conditioned on its utterance's
    previous windows: the rows of a pass carry prompts of different lengths, and which rows share a pass differs per schedule."""
    from whisper_mojo_amd import synth
    lengths = [9000, 4400, 2100, 6500, 3100]
    mels = [synth.synth_long_mel(tiny_cfg, 70 + b, n) for b, n in enumerate(lengths)]
    kw = dict(prompt=(50258, 50259, 50359), eot=50257, max_loop=30, timestamps=(50364, 50363, 50), condition_on_prev_tokens=True,
              prompt_ids=[50361, 2425, 11, 1002])
    m2 = make_model(tiny_cfg, tiny_weights, max_batch=2)
    got2, st2 = m2.transcribe_long_form(mels, return_stats=True, **kw)
    alone = [m2.transcribe_long_form([x], **kw)[0] for x in mels]
    cold = m2.transcribe_long_form(mels, prompt=kw["prompt"], eot=50257, max_loop=30, timestamps=kw["timestamps"])
    m2.close()
    m8 = make_model(tiny_cfg, tiny_weights, max_batch=8)
    got8, st8 = m8.transcribe_long_form(mels, return_stats=True, **kw)
    m8.close()
    assert_same(got2, alone)
    assert_same(got2, got8)
    assert (st2["windows"], st2["stalled"]) == (st8["windows"], st8["stalled"])
    assert any(x["sequence"] != y["sequence"] for x, y in zip(got2, cold))  # conditioning did change something


def test_zero_options_are_wm_transcribe_long(hip, tiny_cfg, tiny_weights):
    from whisper_mojo_amd import _lib, synth
    lengths = [7000, 2500, 4100]
    feats = np.zeros((3, tiny_cfg.n_mels, max(lengths)), np.float32)
    for b, n in enumerate(lengths):
        feats[b, :, :n] = synth.synth_long_mel(tiny_cfg, 80 + b, n)
    m = make_model(tiny_cfg, tiny_weights, max_batch=4)
    opts, _keep = m._opts((50258, 50259, 50359), 50257, 30, False, timestamps=(50364, 50363, 50))
    nf = np.asarray(lengths, np.int32)
    ip = C.POINTER(C.c_int32)
    L = _lib.lib()

    def run(fn, *extra):
        h = C.c_void_p()
        _lib.check(fn(m._h, C.c_void_p(feats.ctypes.data), 0, 3, feats.shape[2], nf.ctypes.data_as(ip), C.byref(opts), *extra, C.byref(h)))
        return _lib.long_result(h, 3)

    base, st = run(L.wm_transcribe_long)
    for lo in (None, C.byref(_lib.WmLongOpts(0, 0, None, 0, 0)), C.byref(_lib.WmLongOpts(0, 50361, None, 0, 0))):
        got, st2 = run(L.wm_transcribe_long_ex, lo)
        assert_same(got, base)
        assert st2 == st
    # refused before the first window: the longest possible prompt does not fit, all-segments without conditioning
    big, _k = m._opts((50258, 50259, 50359), 50257, 230, False, timestamps=(50364, 50363, 50))
    h = C.c_void_p()
    cond = _lib.WmLongOpts(1, 50361, None, 0, 0)
    assert L.wm_transcribe_long_ex(m._h, C.c_void_p(feats.ctypes.data), 0, 3, feats.shape[2], nf.ctypes.data_as(ip), C.byref(big), C.byref(cond),
                                   C.byref(h)) == -1
    pid = np.asarray([50361, 5, 6], np.int32)
    bad = _lib.WmLongOpts(0, 50361, pid.ctypes.data_as(ip), 3, 1)
    assert L.wm_transcribe_long_ex(m._h, C.c_void_p(feats.ctypes.data), 0, 3, feats.shape[2], nf.ctypes.data_as(ip), C.byref(opts), C.byref(bad),
                                   C.byref(h)) == -1
    got, st2 = run(L.wm_transcribe_long_ex, None)
    assert_same(got, base)
    m.close()
