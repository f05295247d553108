"""GPU: long-form transcription with language detection (wm_transcribe_long_lang) against real HF
generate(..., language=None, return_segments=True) runs (tests/golden/lang_detect_tiny_hf.npz, every recording run alone,
tools/make_golden_lang.py): the detected languages, sequences, segment counts, start and end bit for bit, for the plain and the
condition_on_prev_tokens case; and the result equals transcribe_long_form with each recording's language given by hand."""
import numpy as np
import pytest

from test_gpu_lang_detect import hip, setup  # noqa: F401
from test_gpu_long_form import assert_same, make_model
from test_long_prompt import assert_matches_fixture

pytestmark = pytest.mark.gpu


def _case(case):
    from whisper_mojo_amd import synth
    cfg, w, z, _rows, lang_ids = setup("tiny")
    ramp = np.linspace(-1, 1, cfg.n_mels, dtype=np.float32)[:, None]
    lengths = [int(v) for v in z[f"{case}_lengths"]]
    mels, langs = [], []
    for b, n in enumerate(lengths):
        k = f"{case}_u{b}_"
        g, t = np.float32(z[k + "gain"]), np.float32(z[k + "tilt"])
        mels.append((g * synth.synth_long_mel(cfg, int(z[k + "seed"]), n) - (np.float32(1) - g) + t * ramp).astype(np.float32))
        langs.append(int(z[k + "lang"]))
    kw = dict(eot=int(z["eos"]), max_loop=int(z["l_max_new"]) - 1, suppress_tokens=z["s_suppress"].tolist(),
              begin_suppress_tokens=z["s_begin_suppress"].tolist(), timestamps=(int(z["timestamp_begin"]), int(z["no_ts"]), int(z["s_max_init"])),
              condition_on_prev_tokens=bool(z[f"{case}_cond"]), prev_sot_token=int(z["no_ts"]) - 2)
    return cfg, w, z, lang_ids, mels, lengths, langs, kw


def test_fixture_has_both_cases_and_two_languages():
    _cfg, _w, z, _rows, _ids = setup("tiny")
    cases = [str(c) for c in z["l_cases"]]
    assert cases == ["plain", "cond"] and int(z["plain_cond"]) == 0 and int(z["cond_cond"]) == 1
    langs = [int(z[f"{c}_u{b}_lang"]) for c in cases for b in range(len(z[f"{c}_lengths"]))]
    assert len(set(langs)) >= 2 and min(float(z[f"{c}_u{b}_gap"]) for c in cases for b in range(len(z[f"{c}_lengths"]))) >= 1e-2


@pytest.mark.parametrize("case", ["plain", "cond"])
@pytest.mark.parametrize("max_batch", [2, 8])
def test_matches_hf_generate_with_language_none(hip, case, max_batch):
    cfg, w, z, lang_ids, mels, lengths, langs, kw = _case(case)
    init = z["init"].tolist()
    other = next(t for t in lang_ids if t not in langs)
    m = make_model(cfg, w, max_batch=max_batch)
    got, st, lang = m.transcribe_long_form(mels, prompt=[init[0], other, init[2]], detect_language=lang_ids, return_stats=True, **kw)
    assert lang.tolist() == langs
    assert_matches_fixture(got, z, case, len(lengths))
    assert st["row_passes"] == st["passes"]  # every pass takes the per-row route
    by_hand = [m.transcribe_long_form([x], prompt=[init[0], langs[b], init[2]], **kw)[0] for b, x in enumerate(mels)]
    assert_same(got, by_hand)
    alone = [m.transcribe_long_form([x], prompt=init, detect_language=lang_ids, **kw) for x in mels]
    assert_same(got, [a[0][0] for a in alone])
    assert [int(a[1][0]) for a in alone] == langs
    m.close()


def test_pcm_entry_and_refusals(hip):
    from whisper_mojo_amd import frontend
    cfg, w, z, lang_ids, _mels, _lengths, _langs, kw = _case("plain")
    init = z["init"].tolist()
    m = make_model(cfg, w, max_batch=2)
    r = np.random.default_rng(3)
    audios = [(0.1 * r.standard_normal(n)).astype(np.float32) for n in (16000 * 35, 16000 * 8)]
    got, lang = frontend.transcribe_audio_long_form(m, audios, prompt=init, detect_language=lang_ids, **kw)
    assert len(got) == 2 and all(int(t) in lang_ids for t in lang)
    by_hand = [frontend.transcribe_audio_long_form(m, [a], prompt=[init[0], int(lang[b]), init[2]], **kw)[0] for b, a in enumerate(audios)]
    assert_same(got, by_hand)
    with pytest.raises(ValueError):
        m.transcribe_long_form(_mels, prompt=init[:1], detect_language=lang_ids, **kw)
    with pytest.raises(ValueError):
        m.transcribe_long_form(_mels, prompt=init, detect_language=[50259, 50259], **kw)
    m.close()
