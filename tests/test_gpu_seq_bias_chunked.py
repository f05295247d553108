"""Chunked long-form transcription with sequence_bias / bad_words_ids (-m gpu): the library's chunk scheduler equals
the per-chunk loop of tests/test_gpu_chunked.py — every chunk decoded on its own with the same lists, the ids merged by the numpy
restatement of the stitch — so every chunk's pass sees that chunk's decoder ids only."""
import pytest

from test_gpu_chunked import CHUNK_S, FIRST_SPECIAL, KW, check, chunk_refs, hip, model, recordings  # noqa: F401

pytestmark = pytest.mark.gpu


def test_sequence_options_per_chunk(model, hip, recordings):
    from whisper_mojo_amd import frontend
    audios = [recordings["30s"][:100000], recordings["0.5s"]]
    plain = chunk_refs(model, hip, audios)
    g = plain[0][0][1][len(KW["prompt"]):]  # the ids the first chunk generates without the lists (all distinct: KW's n-gram size is 1)
    tab = dict(KW, bad_words_ids=[[g[1], g[2]], [g[5]], [KW["prompt"][-1], g[0], 7]],
               sequence_bias={(g[0], 7): 2.0, (KW["prompt"][-1], g[0], 7): 0.5, (g[8],): float("-inf"), (9,): 1.0})
    ref = chunk_refs(model, hip, audios, call=lambda group: model.transcribe_batch(frontend.log_mel(model, group), **tab))
    got = model.transcribe_chunked(audios, CHUNK_S, return_chunks=True, first_special=FIRST_SPECIAL, **tab)
    check(got, ref)
    assert ref != plain  # the lists did change what was decoded
    assert all(g[5] not in ids[len(KW["prompt"]):] and g[8] not in ids[len(KW["prompt"]):] for r in ref for _, ids in r)
    check(model.transcribe_chunked(audios, CHUNK_S, return_chunks=True, first_special=FIRST_SPECIAL, **KW), plain)  # and were switched off again
