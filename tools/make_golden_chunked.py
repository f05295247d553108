"""Writes tests/golden/chunked_hf.npz (data only, a few KB): what the installed transformers gives for the two host-visible halves of
chunked long-form transcription.  Run on the CPU:

    python tools/make_golden_chunked.py

Chunk tables: AutomaticSpeechRecognitionPipeline.preprocess — HF's seconds -> samples rounding, its stride check and its real
chunk_iter — driven with a stub feature extractor that records where each chunk starts (chunk_iter reports the length and the strides
only).  Merge cases: tokenization_whisper._find_longest_common_sequence(sequences) on id lists stripped as _decode_asr strips them
(every id >= first_special dropped, an empty list is no operand)."""
from __future__ import annotations

import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "chunked_hf.npz")
SR = 16000
FIRST_SPECIAL = 50257

LENGTHS = [1, 8000, 479999, 480000, 480001, 800000, 800001, 1120000, 5000000]
# (chunk_length_s, stride_length_s as the pipeline takes it)
STRIDES = {"default": (30.0, None), "zero": (30.0, (0.0, 0.0)), "asym": (30.0, (3.0, 7.0)), "raises": (30.0, (16.0, 16.0))}


def hf_table(T, chunk_length_s, stride_length_s):
    """-> int32 [n, 5] of (start, len, stride_left, stride_right, is_last), or None when HF raises"""
    from transformers.pipelines.automatic_speech_recognition import AutomaticSpeechRecognitionPipeline as P

    starts = []

    def extractor(chunk, **kw):
        starts.append(int(chunk[0]))
        return {}

    extractor.sampling_rate = SR
    stub = types.SimpleNamespace(feature_extractor=extractor, _align_to=1, dtype=None, type="seq2seq_whisper")
    try:
        items = list(P.preprocess(stub, np.arange(T, dtype=np.int64), chunk_length_s, stride_length_s))
    except ValueError:
        return None
    rows = []
    for it in items:
        ln, sl, sr = it["stride"]
        rows.append((None, ln, sl, sr, int(it["is_last"])))
    # chunk_iter calls the extractor for every chunk it visits, also the one it does not yield (len <= stride_left): a yielded chunk
    # is the visited start whose len = min(T, start + chunk_len) - start fits the next yielded stride
    chunk_len = int(round(chunk_length_s * SR))
    table = []
    k = 0
    for st in starts:
        ln = min(T, st + chunk_len) - st
        if k < len(rows) and rows[k][1] == ln and (k == 0) == (st == 0):
            table.append((st, ln, rows[k][2], rows[k][3], rows[k][4]))
            k += 1
    assert k == len(rows), (T, starts, rows)
    return np.asarray(table, np.int32).reshape(-1, 5)


def merge_cases():
    """name -> list of chunks (id lists, specials included where the case is about the strip)"""
    rng = np.random.default_rng(30)
    c = {}

    def overlap(n_left, n_right, n_ov, base=100):
        a = list(range(base, base + n_left))
        return [a, a[n_left - n_ov:] + list(range(base + 5000, base + 5000 + n_right - n_ov))]

    c["clean_overlap_2"] = overlap(9, 8, 2)
    c["clean_overlap_5"] = overlap(12, 11, 5)
    c["clean_overlap_40"] = overlap(90, 70, 40)
    sub = overlap(30, 30, 11)
    sub[1][5] = 49999  # one substituted id inside the overlap: fault tolerance
    c["one_substitution"] = sub
    c["single_match_no_merge"] = [[1, 2, 3, 4], [4, 5, 6]]
    c["eps_decides"] = [[10, 11, 1, 2, 1, 2], [1, 2, 1, 2, 20, 21]]  # i = 2 and i = 4 both score matches / i = 1
    left = list(range(1000, 1200))
    right = list(range(2000, 2200))
    right[150], right[160] = left[150], left[160]  # i = 200: 2 / 200 + 200 / 10000
    right[10], right[20] = left[110], left[120]    # i = 100: 2 / 100 + 100 / 10000, the same double
    c["exact_tie_lowest_i"] = [left, right]
    c["no_overlap"] = [[1, 2, 3, 4, 5], [6, 7, 8, 9]]
    c["left_longer"] = overlap(60, 9, 4)
    c["right_longer"] = overlap(7, 80, 3)
    c["right_len_1"] = [[5, 6, 7, 8], [8]]
    c["empty_middle"] = [list(range(300, 320)), [], list(range(315, 340))]
    c["empty_end"] = [list(range(300, 320)), list(range(315, 340)), []]
    c["single_chunk"] = [list(range(40, 60))]
    c["chain_6"] = [list(range(10 * k, 10 * k + 15)) for k in range(6)]
    a = rng.integers(0, 50000, 448).tolist()
    c["L448_R448"] = [a, a[408:] + rng.integers(0, 50000, 408).tolist()]
    text = rng.integers(0, FIRST_SPECIAL, 60).tolist()

    def with_specials(ids, lang=50259):
        out = [50258, lang, 50359, 50363]
        for j, t in enumerate(ids):
            out.append(t)
            if j % 7 == 3:
                out.append(int(rng.integers(50364, 51865)))  # a timestamp id in the middle
        return out + [50257]

    c["strip_specials"] = [with_specials(text[:35]), with_specials(text[25:]), [50258, 50259, 50359, 50363, 51864, 50257]]
    c["all_special"] = [[50258, 50259, 50257], [50257]]
    c["batch_rec_1"] = [rng.integers(0, 50000, 17).tolist()]
    b4 = rng.integers(0, 50000, 100).tolist()
    c["batch_rec_4"] = [b4[20 * k:20 * k + 32] for k in range(4)]
    b9 = rng.integers(0, 50000, 200).tolist()
    c["batch_rec_9"] = [b9[20 * k:20 * k + 30] + ([50257] if k % 2 else []) for k in range(9)]
    return c


def hf_merge(chunks):
    from transformers.models.whisper.tokenization_whisper import _find_longest_common_sequence
    seqs = [[t for t in ch if t < FIRST_SPECIAL] for ch in chunks]
    seqs = [s for s in seqs if s]  # `if current_tokens:`
    return [int(t) for t in _find_longest_common_sequence(seqs)] if seqs else []


def main():
    import transformers
    out = {"transformers_version": np.asarray(transformers.__version__), "first_special": np.asarray(FIRST_SPECIAL, np.int32),
           "lengths": np.asarray(LENGTHS, np.int64), "stride_names": np.asarray(list(STRIDES))}
    for name, (cl, st) in STRIDES.items():
        from whisper_mojo_amd import _lib
        out[f"samples_{name}"] = np.asarray(_lib.chunk_strides(cl, st, SR), np.int64)  # checked against HF's own rounding below
        raised = []
        for T in LENGTHS:
            tab = hf_table(T, cl, st)
            raised.append(tab is None)
            if tab is not None:
                out[f"table_{name}_{T}"] = tab
        out[f"raises_{name}"] = np.asarray(raised)
        assert all(raised) or not any(raised)
    names = []
    for name, chunks in merge_cases().items():
        names.append(name)
        out[f"merge_{name}_ids"] = np.asarray([t for ch in chunks for t in ch], np.int32)
        out[f"merge_{name}_lens"] = np.asarray([len(ch) for ch in chunks], np.int32)
        out[f"merge_{name}_want"] = np.asarray(hf_merge(chunks), np.int32)
    out["merge_names"] = np.asarray(names)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes;", len(names), "merge cases")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    main()
