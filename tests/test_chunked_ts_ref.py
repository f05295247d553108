"""CPU: the timestamp stitch of chunked long-form transcription against the installed transformers' own results,
recorded by tools/make_golden_chunked_ts.py in tests/golden/chunked_ts_hf.npz.

segments_ref below restates tokenization_whisper._decode_asr with return_timestamps=True / "word" (language fields, the split at a
language change and _strip_prompt left out) and _find_longest_common_sequence(sequences, token_timestamp_sequences), folded as the
operands arrive.  It is the reference of the GPU tests (tests/test_gpu_chunk_segments_op.py, tests/test_gpu_chunked_ts.py), pinned
to HF by the fixture: the GPU machine need not have transformers.  Every time is a Python float (float64) and every operation is
the one HF performs, in HF's order, so the comparison is on the bits.

The knobs of segments_ref switch one rule each to what a wrong kernel would do; test_every_rule_decides_its_case shows that every
rule decides the answer of the case the fixture holds for it.  collate_words (whisper_mojo_amd.tokenizer) is compared with HF's
_collate_word_timestamps where transformers is installed."""
import json
import math
import os
import struct

import numpy as np
import pytest

from conftest import GOLDEN, golden
from whisper_mojo_amd.tokenizer import Tokenizer, collate_words

SR = 16000
MODES = ("segments", "word")


def round2(x, py=True):
    """Python's round(x, 2); py=False: the rint(x * 100) / 100 a kernel might be tempted by"""
    return round(x, 2) if py else float(np.rint(np.float64(x) * np.float64(100.0)) / np.float64(100.0))


def merge_fold(left, right, word, pair_cmp="le"):
    """one step of _find_longest_common_sequence: (ids, pairs) x (ids, pairs) -> (emitted ids, emitted pairs, new left)"""
    lid, lp = left
    rid, rp = right
    L, R = len(lid), len(rid)
    best, idx = 0.0, (L, L, 0, 0)
    for i in range(1, L + R):
        ls, le = max(0, L - i), min(L, L + R - i)
        rs, re = max(0, i - L), min(R, i)
        matches = 0
        for j in range(le - ls):
            if lid[ls + j] != rid[rs + j]:
                continue
            if word and pair_cmp == "le" and not (lp[ls + j] <= rp[rs + j]):
                continue
            if word and pair_cmp == "lt" and not (lp[ls + j] < rp[rs + j]):
                continue
            matches += 1
        score = matches / i + i / 10000.0
        if matches > 1 and score > best:
            best, idx = score, (ls, le, rs, re)
    ls, le, rs, re = idx
    lm, rm = (le + ls) // 2, (re + rs) // 2
    return lid[:lm], lp[:lm], (rid[rm:], rp[rm:])


def segments_ref(chunks, word, timestamp_begin, first_special, time_precision, segment_size, pair_cmp="le", keep_skip=True,
                 first_ts_test=True, dup_end=True, empty_operand=True, py_round=True, reset=True, stats=None):
    """chunks: [(ids, (len, stride_left, stride_right) in samples, token times or None)] of one recording, in order ->
    [{"timestamp": (start, end | None), "ids": [...], "token_timestamps": [(s, e), ...]}] ("token_timestamps" in word mode only).
    stats: a dict that receives "closed", "skipped" and "overlaps" (what the end-to-end test asserts before it compares)."""
    st = stats if stats is not None else {}
    for k in ("closed", "skipped", "overlaps"):
        st.setdefault(k, 0)
    segs = []
    start = None        # chunk["timestamp"][0]
    n_ops = 0           # len(previous_tokens)
    any_ids = False     # any(p for p in previous_tokens)
    left = ([], [])
    out_ids, out_pairs = [], []
    time_offset = 0.0
    skip = False

    def operand(ids, pairs):
        nonlocal n_ops, any_ids, left
        if n_ops == 0:
            left = (ids, pairs)
        else:
            a, b, new_left = merge_fold(left, (ids, pairs), word, pair_cmp)
            if len(a) < len(left[0]) or len(new_left[0]) < len(ids):
                st["overlaps"] += 1
            out_ids.extend(a)
            out_pairs.extend(b)
            left = new_left
        n_ops += 1
        any_ids = any_ids or bool(ids)

    def flush(end):
        nonlocal n_ops, any_ids, left, out_ids, out_pairs, start
        seg = {"timestamp": (start, end), "ids": out_ids + left[0]}
        if word:
            seg["token_timestamps"] = out_pairs + left[1]
        segs.append(seg)
        n_ops, any_ids, left, out_ids, out_pairs, start = 0, False, ([], []), [], [], None

    for ids, (ln, sl, sr), tt in chunks:
        ids = [int(t) for t in ids]
        chunk_len, stride_left, stride_right = ln / SR, sl / SR, sr / SR
        last_timestamp = None
        first_timestamp = timestamp_begin
        cur_max, prev_len, penultimate = 0.0, 0.0, 0.0
        time_offset -= stride_left
        right_start = chunk_len - stride_right
        if stride_left:
            first_timestamp = stride_left / time_precision + timestamp_begin
        if stride_right:
            for t in reversed(ids):
                if t >= timestamp_begin:
                    if last_timestamp is not None and (t - timestamp_begin) * time_precision < right_start:
                        break
                    last_timestamp = t
        cur_ids, cur_pairs = [], []
        for i, t in enumerate(ids):
            if first_special <= t < timestamp_begin:
                continue
            if t >= timestamp_begin:
                ts = float((t - timestamp_begin) * time_precision)
                if ts < cur_max:
                    single = i >= 2 and not (ids[i - 1] >= timestamp_begin and ids[i - 2] >= timestamp_begin)
                    if single:
                        prev_len += time_precision * segment_size
                    else:
                        cur_max = penultimate
                        prev_len += penultimate
                penultimate = cur_max
                cur_max = ts
                time = round2((t - timestamp_begin) * time_precision + time_offset + prev_len, py_round)
                if last_timestamp and t >= last_timestamp:
                    skip = True
                    st["skipped"] += 1
                elif skip or (first_ts_test and n_ops > 0 and t < first_timestamp):
                    if not skip:
                        st["skipped"] += 1
                    skip = False
                elif start is None:
                    start = time
                elif dup_end and time == start:
                    pass
                else:
                    # (an empty current_tokens never changes the merged ids; what it decides is that a segment without ids, closed
                    # with nothing pending, exists at all — a kernel that drops empty operands as chunk_merge_kernel does loses it)
                    if empty_operand or cur_ids:
                        operand(cur_ids, cur_pairs)
                    st["closed"] += 1
                    if n_ops:
                        flush(time)
                    else:
                        start = None
                    cur_ids, cur_pairs = [], []
            else:
                cur_ids.append(t)
                if word:
                    s = round2(0.0 + time_offset, py_round) if i == 0 else round2(float(np.float32(tt[i - 1])) + time_offset, py_round)
                    cur_pairs.append((s, round2(float(np.float32(tt[i])) + time_offset, py_round)))
        time_offset += chunk_len - stride_right
        if not keep_skip:
            skip = False
        if cur_ids:
            operand(cur_ids, cur_pairs)
        elif reset and not any_ids:
            n_ops, any_ids, left, out_ids, out_pairs, start = 0, False, ([], []), [], [], None
    if n_ops:
        flush(None)
    return segs


# ---- the fixture ------------------------------------------------------------------------------------------------------------------
def case_names(g):
    return [str(n) for n in g["names"]]


def case_input(g, name, word):
    """-> (chunks as segments_ref takes them, params dict)"""
    ids, lens = g[f"{name}_ids"].tolist(), g[f"{name}_lens"].tolist()
    strides = g[f"{name}_strides"].tolist()
    tt = g[f"{name}_times"]
    chunks, k = [], 0
    for n, s in zip(lens, strides):
        chunks.append((ids[k:k + n], tuple(s), tt[k:k + n] if word else None))
        k += n
    tb, fs, seg = (int(v) for v in g[f"{name}_params"])
    return chunks, dict(timestamp_begin=tb, first_special=fs, time_precision=float(g[f"{name}_tp"]), segment_size=seg)


def case_want(g, name, mode):
    """-> segments as segments_ref returns them, from the arrays HF's run left"""
    times, rng, ids = g[f"{name}_{mode}_seg_times"], g[f"{name}_{mode}_seg_range"].tolist(), g[f"{name}_{mode}_ids"].tolist()
    pairs = g[f"{name}_{mode}_pairs"] if mode == "word" else None
    out = []
    for (s, e), (b0, b1) in zip(times.tolist(), rng):
        seg = {"timestamp": (None if math.isnan(s) else s, None if math.isnan(e) else e), "ids": ids[b0:b1]}
        if pairs is not None:
            seg["token_timestamps"] = [tuple(p) for p in pairs[b0:b1].tolist()]
        out.append(seg)
    return out


def bits(x):
    return None if x is None else struct.pack("<d", x)


def seg_bits(segs):
    """segments with every time as its float64 bit pattern: equality on this is equality bit for bit (0.0 against -0.0 included)"""
    return [(bits(s["timestamp"][0]), bits(s["timestamp"][1]), s["ids"],
             [(bits(a), bits(b)) for a, b in s["token_timestamps"]] if "token_timestamps" in s else None) for s in segs]


REQUIRED = ["single_two_segments", "three_chunks_left", "three_chunks_right", "three_chunks_both", "right_last_skipped_with_pair",
            "end_equals_start", "no_end_timestamp", "empty_current_at_close", "all_empty_reset", "reset_forgets_start", "reset_forgets_start_strided", "decreasing_single_ending",
            "decreasing_double_ending", "odd_samples_half", "pair_out_of_order", "equal_starts_ends_decide", "operands_448",
            "batch_rec_1", "batch_rec_4", "batch_rec_9"]


def test_fixture_holds_the_required_cases():
    g = golden("chunked_ts_hf")
    assert set(REQUIRED) <= set(case_names(g))
    assert [len(g[f"batch_rec_{n}_lens"]) for n in (1, 4, 9)] == [1, 4, 9]
    assert int(g["operands_448_lens"].max()) >= 448


@pytest.mark.parametrize("mode", MODES)
def test_segments_ref_matches_hf(mode):
    g = golden("chunked_ts_hf")
    for name in case_names(g):
        chunks, par = case_input(g, name, mode == "word")
        assert seg_bits(segments_ref(chunks, mode == "word", **par)) == seg_bits(case_want(g, name, mode)), name


def test_word_mode_merge_differs_from_the_plain_merge():
    """the case the fixture holds for the pair comparison: the same ids merge differently once the pairs are looked at"""
    g = golden("chunked_ts_hf")
    name = "pair_out_of_order"
    w = [t for s in case_want(g, name, "word") for t in s["ids"]]
    p = [t for s in case_want(g, name, "segments") for t in s["ids"]]
    assert w != p


def test_a_time_sits_on_a_half():
    """odd_samples_half: chunk and stride lengths that are no multiples of 160 samples, and a time whose hundredths lie within 1e-9 of
    a half before it is rounded"""
    from fractions import Fraction
    g = golden("chunked_ts_hf")
    chunks, par = case_input(g, "odd_samples_half", True)
    assert any(v % 160 for _, s, _ in chunks for v in s)
    off, near = 0.0, 0
    for ids, (ln, sl, sr), tt in chunks:
        off -= sl / SR
        for i, t in enumerate(ids):
            if t < par["first_special"]:
                x = Fraction(float(np.float32(tt[i])) + off) * 100
                near += abs(x - math.floor(x) - Fraction(1, 2)) < Fraction(1, 10 ** 9)
        off += ln / SR - sr / SR
    assert near >= 1


KNOBS = [("pair_out_of_order", "word", dict(pair_cmp="none")), ("equal_starts_ends_decide", "word", dict(pair_cmp="lt")),
         ("right_last_skipped_with_pair", "segments", dict(keep_skip=False)), ("three_chunks_left", "segments", dict(first_ts_test=False)),
         ("end_equals_start", "segments", dict(dup_end=False)), ("empty_current_at_close", "segments", dict(empty_operand=False)),
         ("rounding_ties", "word", dict(py_round=False)), ("rounding_ties", "segments", dict(py_round=False)),
         ("reset_forgets_start", "segments", dict(reset=False)), ("reset_forgets_start", "word", dict(reset=False)),
         ("reset_forgets_start_strided", "segments", dict(reset=False)), ("reset_forgets_start_strided", "word", dict(reset=False))]


@pytest.mark.parametrize("case, mode, knob", KNOBS)
def test_every_rule_decides_its_case(case, mode, knob):
    g = golden("chunked_ts_hf")
    chunks, par = case_input(g, case, mode == "word")
    want = seg_bits(case_want(g, case, mode))
    assert seg_bits(segments_ref(chunks, mode == "word", **par)) == want
    assert seg_bits(segments_ref(chunks, mode == "word", **par, **knob)) != want


# ---- word grouping ------------------------------------------------------------------------------------------------------------------
class HFTokenizerView:
    """what _collate_word_timestamps asks of a tokenizer, over the project's Tokenizer"""
    language = None

    def __init__(self, tok, eos):
        self.tok, self.eos_token_id = tok, eos

    def decode(self, ids, decode_with_timestamps=False, **kw):
        return self.tok.decode_text(ids)


def word_cases(vocab):
    ids = sorted(vocab)
    rng = np.random.default_rng(31)
    cases = [[int(t) for t in rng.choice(ids, n)] for n in (1, 2, 7, 30, 60)]
    by_text = {v: k for k, v in vocab.items()}
    picks = [by_text[t] for t in ("Ġ\"", "Ġ(", "Ġ-", ".", ",", "!", "?", "'", ")", "Ġthe", "Ġa") if t in by_text]
    if picks:
        cases.append([int(t) for t in rng.choice(picks + ids[:40], 50)])
    return cases


def test_collate_words_equals_hf():
    tw = pytest.importorskip("transformers.models.whisper.tokenization_whisper")
    with open(os.path.join(GOLDEN, "vocab_subset.json"), encoding="utf-8") as f:
        vocab = {int(k): v for k, v in json.load(f)["tokens"].items()}
    text = {k: v for k, v in vocab.items() if not Tokenizer._is_special(v)}
    tok = Tokenizer(vocab)
    view = HFTokenizerView(tok, eos=50257)
    seen = 0
    for ids in word_cases(text):
        pairs = [(round(0.02 * j, 2), round(0.02 * j + 0.02, 2)) for j in range(len(ids))]
        want = tw._collate_word_timestamps(view, ids, pairs, "english", False)
        got = collate_words(tok, ids, pairs)
        assert got == [{"text": w["text"], "timestamp": w["timestamp"]} for w in want], ids
        seen += len(got)
    assert seen > 20
    with pytest.raises(NotImplementedError):
        collate_words(tok, [1, 2], [(0.0, 0.1), (0.1, 0.2)], language="japanese")
