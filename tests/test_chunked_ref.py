"""CPU: the host halves of chunked long-form transcription against the installed transformers' own results, recorded
by tools/make_golden_chunked.py in tests/golden/chunked_hf.npz:

  * wm_chunk_table against the chunks of AutomaticSpeechRecognitionPipeline.preprocess / chunk_iter, the raising stride pair as
    WM_E_ARG;
  * merge_ref below — a numpy restatement of _decode_asr's strip followed by _find_longest_common_sequence(sequences) — against
    every recorded merge.  It is the reference of the GPU tests (tests/test_gpu_chunk_ops.py, tests/test_gpu_chunked.py), pinned to HF
    by the fixture: the GPU machine need not have transformers.

The knobs of merge_ref switch one rule each to what a wrong kernel would do; the last test shows that every rule decides the answer
of the case the fixture holds for it."""
import numpy as np
import pytest

from conftest import golden

FIRST_SPECIAL = 50257


def strip(chunk, first_special=FIRST_SPECIAL):
    return [int(t) for t in chunk if 0 <= int(t) < first_special]


def merge_ref(chunks, first_special=FIRST_SPECIAL, min_matches=2, eps=True, tie_low=True, replace_left=True):
    """chunks: the id lists of one recording's chunks, in order -> the merged ids.  Float64 throughout, as Python computes."""
    seqs = [s for s in (strip(c, first_special) for c in chunks) if s]
    if not seqs:
        return []
    left = np.asarray(seqs[0], np.int64)
    total = []
    for right in seqs[1:]:
        right = np.asarray(right, np.int64)
        L, R = len(left), len(right)
        best, idx = np.float64(0.0), (L, L, 0, 0)
        for i in range(1, L + R):
            ls, le = max(0, L - i), min(L, L + R - i)
            rs, re = max(0, i - L), min(R, i)
            matches = int(np.sum(left[ls:le] == right[rs:re]))
            score = np.float64(matches) / np.float64(i) + (np.float64(i) / np.float64(10000.0) if eps else np.float64(0.0))
            if matches >= min_matches and (score > best if tie_low else score >= best):
                best, idx = score, (ls, le, rs, re)
        ls, le, rs, re = idx
        total += left[:(le + ls) // 2].tolist()
        if replace_left:
            left = right[(re + rs) // 2:]
    return total + left.tolist()


def fixture_chunks(g, name):
    ids, lens = g[f"merge_{name}_ids"].tolist(), g[f"merge_{name}_lens"].tolist()
    out, k = [], 0
    for n in lens:
        out.append(ids[k:k + n])
        k += n
    return out


def merge_names(g):
    return [str(n) for n in g["merge_names"]]


def test_chunk_table_matches_hf():
    from whisper_mojo_amd import _lib
    g = golden("chunked_hf")
    seen = 0
    for name in (str(n) for n in g["stride_names"]):
        chunk_len, sl, sr = (int(v) for v in g[f"samples_{name}"])
        for T, raised in zip(g["lengths"].tolist(), g[f"raises_{name}"].tolist()):
            if raised:
                with pytest.raises(_lib.WhisperMiError, match="libwhispermi error -1"):  # WM_E_ARG
                    _lib.chunk_table([T], chunk_len, sl, sr)
                continue
            got = _lib.chunk_table([T], chunk_len, sl, sr)
            assert (got[:, 0] == 0).all()
            assert got[:, 1:].tolist() == g[f"table_{name}_{T}"].tolist(), (name, T)
            seen += 1
    assert seen == 27  # nine lengths under the default, the (0, 0) and the (3 s, 7 s) strides


def test_chunk_table_default_strides_and_seconds():
    from whisper_mojo_amd import _lib
    g = golden("chunked_hf")
    assert _lib.chunk_strides(30.0, None) == tuple(int(v) for v in g["samples_default"]) == (480000, 80000, 80000)
    assert _lib.chunk_strides(30.0, (3.0, 7.0)) == tuple(int(v) for v in g["samples_asym"])
    assert _lib.chunk_table([800001]).tolist() == _lib.chunk_table([800001], 480000, 80000, 80000).tolist()


def test_chunk_table_several_recordings_and_refusals():
    from whisper_mojo_amd import _lib
    g = golden("chunked_hf")
    lens = [800001, 0, 1, 1120000]
    got = _lib.chunk_table(lens, 480000, 80000, 80000)
    want = []
    for r, T in enumerate(lens):
        if T:
            want += [[r] + row for row in g[f"table_default_{T}"].tolist()]
    assert got.tolist() == want
    with pytest.raises(_lib.WhisperMiError, match="window"):
        _lib.chunk_table([100000], 480000, 80000, 80000, window=32000)
    with pytest.raises(_lib.WhisperMiError):  # step 0: HF's chunk_iter dies in range(0, n, 0)
        _lib.chunk_table([100000], 32000, 16000, 16000)
    assert _lib.chunk_table([100000], 32000, 0, 0, window=32000).shape == (4, 6)


def test_merge_ref_matches_hf():
    g = golden("chunked_hf")
    assert int(g["first_special"]) == FIRST_SPECIAL
    names = merge_names(g)
    assert len(names) >= 20
    for name in names:
        assert merge_ref(fixture_chunks(g, name)) == g[f"merge_{name}_want"].tolist(), name


@pytest.mark.parametrize("case, knob", [("single_match_no_merge", dict(min_matches=1)), ("eps_decides", dict(eps=False)),
                                        ("exact_tie_lowest_i", dict(tie_low=False)), ("chain_6", dict(replace_left=False))])
def test_every_rule_decides_its_case(case, knob):
    g = golden("chunked_hf")
    chunks = fixture_chunks(g, case)
    want = g[f"merge_{case}_want"].tolist()
    assert merge_ref(chunks) == want
    assert merge_ref(chunks, **knob) != want
