"""Writes tests/golden/chunked_ts_hf.npz (data only, about 100 KB): what the installed transformers gives for the timestamp stitch
of chunked long-form transcription.  Run on the CPU; nothing is downloaded:

    python tools/make_golden_chunked_ts.py

HF's real tokenization_whisper._decode_asr runs with return_timestamps=True and "word" on synthetic model outputs (ids, the stride
in seconds as the pipeline's postprocess leaves it, float32 token times), over a duck-typed tokenizer that knows Whisper's id
layout only.  _find_longest_common_sequence is the real one behind a wrapper that records what it returns for every segment (the
resolved ids and pairs) and the segment's timestamp from _decode_asr's own frame; _collate_word_timestamps is replaced by a stub
(word grouping is tested on its own).  Every case is also run through segments_ref of tests/test_chunked_ts_ref.py, and the rules
whose cases the fixture must hold are checked to decide them."""
from __future__ import annotations

import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "chunked_ts_hf.npz")
SR = 16000
FS, TB, TP, SEG = 50257, 50364, 0.02, 1500  # Whisper's multilingual layout: <|endoftext|>, <|0.00|>, 30 s / 1500
PROMPT = [50258, 50259, 50359]
EOT = 50257
FULL, FIRST, MID, LAST = (480000, 0, 0), (480000, 0, 80000), (480000, 80000, 80000), (480000, 80000, 0)


class DuckTokenizer:
    def __init__(self, first_special, timestamp_begin):
        self.fs, self.tb = first_special, timestamp_begin
        self.all_special_ids = list(range(first_special, timestamp_begin))
        self.language = None
        self.eos_token_id = first_special

    def convert_tokens_to_ids(self, tok):
        return {"<|notimestamps|>": self.tb - 1, "<|startofprev|>": self.tb - 3, "<|startoftranscript|>": self.fs + 1}[tok]

    def _strip_prompt(self, ids, prompt_id, start_id):
        return ids

    def decode(self, ids, **kw):
        return "".join("<|s|>" if t >= self.fs else f" {t}" for t in ids)


def hf_segments(chunks, word, tb, fs, tp, seg):
    """chunks: [(ids, (len, sl, sr) samples, float32 times)] -> [(start, end, ids, pairs)] from HF's real _decode_asr"""
    import torch
    from transformers.models.whisper import tokenization_whisper as tw
    real, real_collate = tw._find_longest_common_sequence, tw._collate_word_timestamps
    rec = []

    def merge(sequences, token_timestamp_sequences=None):
        out = real(sequences, token_timestamp_sequences)
        st = sys._getframe(1).f_locals["chunk"]["timestamp"]
        rec.append((st[0], st[1], [int(t) for t in out[0]], [(float(a), float(b)) for a, b in out[1]]))
        return out

    tw._find_longest_common_sequence, tw._collate_word_timestamps = merge, lambda *a, **k: []
    try:
        outs = []
        for ids, (ln, sl, sr), tt in chunks:
            o = {"tokens": torch.tensor([ids], dtype=torch.long), "stride": (ln / SR, sl / SR, sr / SR)}  # postprocess' division
            if word:
                o["token_timestamps"] = torch.tensor(np.asarray(tt, np.float32))[None]
            outs.append(o)
        tw._decode_asr(DuckTokenizer(fs, tb), outs, return_timestamps="word" if word else True, return_language=False, time_precision=tp,
                       segment_size=seg)
    finally:
        tw._find_longest_common_sequence, tw._collate_word_timestamps = real, real_collate
    return rec


def T(x, tb=TB, tp=TP):
    return tb + int(round(x / tp))


def times_for(ids, rng, t0=0.0, step=0.26):
    """increasing float32 token times on HF's 0.02 s grid"""
    t, out = t0, []
    for _ in ids:
        out.append(np.float32(round(t / 0.02) * 0.02))
        t += float(rng.uniform(0.0, step))
    return out


def cases():
    rng = np.random.default_rng(31)
    c = {}
    txt = lambda n: rng.integers(0, 50000, n).tolist()  # noqa: E731

    def put(name, chunks, params=(TB, FS, TP, SEG), times=None):
        rows = []
        for k, (ids, stride) in enumerate(chunks):
            tt = times[k] if times is not None else times_for(ids, rng)
            assert len(tt) == len(ids)
            rows.append((list(ids), stride, np.asarray(tt, np.float32)))
        c[name] = (rows, params)

    a, b, d, e, f, h = txt(9), txt(7), txt(8), txt(6), txt(10), txt(5)
    put("single_two_segments", [(PROMPT + [T(0)] + a + [T(2.4), T(2.4)] + b + [T(5.0), EOT], FULL)])
    # chunk 1 leaves text open; chunk 2 and 3 start with timestamps inside their left stride (< 5 s), which are not split on
    put("three_chunks_left", [(PROMPT + [T(0)] + a + [T(10), T(10)] + b + d, FIRST),
                              (PROMPT + [T(0.5)] + d + [T(7), T(7)] + e + [T(20), T(20)] + f, MID),
                              (PROMPT + [T(1.0), T(1.0)] + f + [T(8), T(8)] + h + [T(12), EOT], LAST)])
    put("three_chunks_right", [(PROMPT + [T(0)] + a + [T(12), T(12)] + b + [T(26), T(26)] + d, FIRST),
                               (PROMPT + [T(6)] + d[3:] + [T(9), T(9)] + e + [T(27.5), T(27.5)] + f, MID),
                               (PROMPT + [T(7.5)] + f[2:] + [T(11), T(11)] + h + [T(14), EOT], LAST)])
    put("three_chunks_both", [(PROMPT + [T(0)] + a + [T(12), T(12)] + b + [T(26), T(26)] + d, FIRST),
                              (PROMPT + [T(1), T(1)] + d + [T(9), T(9)] + e + [T(26.5), T(26.5)] + f + [T(29)], MID),
                              (PROMPT + [T(2)] + f + [T(4.5), T(4.5)] + h + [T(14), EOT], LAST)])
    # one timestamp in the right stride: skipped, and so is the next one, although chunk 2's T(6) lies outside its left stride
    put("right_last_skipped_with_pair", [(PROMPT + [T(0)] + a + [T(13), T(13)] + b + [T(27)], FIRST),
                                         (PROMPT + [T(6)] + d + [T(9), T(9)] + e + [T(15), EOT], LAST)])
    put("end_equals_start", [(PROMPT + [T(2)] + a + [T(2)] + b + [T(4), T(4)] + d + [T(6), EOT], FULL)])
    put("no_end_timestamp", [(PROMPT + [T(0)] + a + b + [EOT], FULL)])
    put("empty_current_at_close", [(PROMPT + [T(0), T(1), T(1)] + a + [T(3), T(3), T(4), EOT], FULL)])
    put("all_empty_reset", [(PROMPT + [T(0)] + a + [T(2), T(2)], FIRST), (PROMPT + [T(6)] + b + [T(8), EOT], LAST)])
    put("decreasing_single_ending", [(PROMPT + [T(0)] + a + [T(10), T(10)] + b + [T(29), T(1)] + d + [T(3), EOT], FULL)])
    put("decreasing_double_ending", [(PROMPT + [T(0)] + a + [T(10), T(10)] + b + [T(20), T(20), T(1)] + d + [T(3), T(3)] + e + [T(2)] + f + [T(4), EOT], FULL)])

    # lengths that are no multiples of 160 samples; 479 999 - 79 999 - 79 920 = 320 080 samples = 20.005 s is chunk 2's time_offset, so
    # every token time that float32 holds exactly (6.0, 6.5, 7.25 ...) lands on x.xx5 up to the last bits of the double sum
    odd = [(479999, 0, 79999), (479999, 79920, 79999), (300001, 79920, 0)]
    halves = [6.0, 6.5, 7.25, 7.26, 8.0, 9.5, 10.75, 10.76, 12.0, 12.5, 13.125, 14.0]
    ids2 = PROMPT + [T(5.5)] + txt(len(halves)) + [T(25)]
    tt2 = [0.0] * 4 + halves + [halves[-1]]
    put("odd_samples_half", [(PROMPT + [T(0)] + a + [T(11), T(11)] + b, odd[0]), (ids2, odd[1]), (PROMPT + [T(5.02)] + d + [T(9), EOT], odd[2])],
        times=[times_for(PROMPT + [0] + a + [0, 0] + b, rng), tt2, times_for(PROMPT + [0] + d + [0, 0], rng)])

    # time_offset 20.005 in chunk 2: every segment time and every pair sits on a half before it is rounded
    n = 40
    words = txt(n)
    ids2 = list(PROMPT)
    ties = [k for k in range(255, 1450) if round(k * TP + 20.005, 2) != float(np.rint((k * TP + 20.005) * 100.0) / 100.0)][:2 * n]
    assert len(ties) == 2 * n
    for k in range(n):  # timestamps whose time, 0.02 k + 20.005, rint(x * 100) / 100 rounds the other way
        ids2 += [TB + ties[2 * k], words[k], TB + ties[2 * k + 1]]
    # the word of segment k is heard at 5.25 + 0.5 k s: float32 holds that exactly, and x.25 + 20.005 is a tie that rint(x * 100) / 100
    # resolves the other way for many k
    tt2 = [0.0] * len(PROMPT) + [v for k in range(n) for v in (5.0 + 0.5 * k, 5.25 + 0.5 * k, 5.25 + 0.5 * k)] + [25.0]
    put("rounding_ties", [(PROMPT + [T(0)] + a + [T(11)], (480080, 0, 80000)), (ids2 + [EOT], (480000, 80000, 0))],
        times=[times_for(PROMPT + [0] + a + [0], rng), tt2])

    # word mode: the overlap's ids are equal, but chunk 2 heard them EARLIER (6.0 + 20 < 27): out of order, so no match
    ov = txt(6)
    ids1 = PROMPT + [T(0)] + a + [T(20), T(20)] + b + ov
    tt1 = times_for(PROMPT + [0] + a + [0, 0] + b, rng) + [np.float32(27.0 + 0.2 * k) for k in range(6)]
    ids2 = PROMPT + [T(5.5)] + ov + d + [T(12), EOT]
    tt2 = [0.0] * 4 + [np.float32(6.0 + 0.2 * k) for k in range(6)] + [np.float32(8 + 0.2 * k) for k in range(len(d) + 2)]
    put("pair_out_of_order", [(ids1, FIRST), (ids2, LAST)], times=[tt1, tt2])
    # two ids overlap: the first with equal pairs, the second with equal starts and the left end below the right one
    ov = txt(2)
    ids1 = PROMPT + [T(0)] + a + [T(20), T(20)] + b + ov
    tt1 = times_for(PROMPT + [0] + a + [0, 0], rng) + [np.float32(25.0 + 0.1 * k) for k in range(len(b) - 1)] + [np.float32(26.0), np.float32(26.2), np.float32(26.4)]
    ids2 = PROMPT + [T(5.5)] + ov + d + [T(12), EOT]
    tt2 = [0.0] * 3 + [np.float32(6.0), np.float32(6.2), np.float32(6.5)] + [np.float32(8 + 0.2 * k) for k in range(len(d) + 2)]
    put("equal_starts_ends_decide", [(ids1, FIRST), (ids2, LAST)], times=[tt1, tt2])

    big = txt(448)
    grid = lambda v: round(v / 0.02) * 0.02  # noqa: E731
    tt1 = [0.0] * 4 + [grid(0.06 * (j + 1)) for j in range(448)]
    tt2 = [0.0] * 4 + [grid(0.06 * (409 + j) - 20.0) for j in range(448)] + [28.0, 28.0]  # the 40 shared ids at the same absolute times
    put("operands_448", [(PROMPT + [T(0)] + big, FIRST), (PROMPT + [T(5.5)] + big[408:] + txt(408) + [T(28), EOT], LAST)], times=[tt1, tt2])

    # the micro model's id layout (vocab 1000: specials from 900, timestamps from 960, a 2 s window of 100 positions)
    tm = lambda x: T(x, 960, 0.02)  # noqa: E731
    sm = rng.integers(0, 900, 30).tolist()
    put("micro_layout", [([950, 951] + [tm(0)] + sm[:8] + [tm(1.0), tm(1.0)] + sm[8:14], (32000, 0, 5333)),
                         ([950, 951] + [tm(0.1)] + sm[10:20] + [tm(1.2), tm(1.2)] + sm[20:26], (32000, 5333, 5333)),
                         ([950, 951] + [tm(0.2)] + sm[22:30] + [tm(1.5), 900], (20000, 5333, 0))], params=(960, 900, 0.02, 100))

    def simulate(n_chunks):
        """a transcript of segments on a time line, heard by overlapping 30 s chunks: each chunk emits the segments it can see,
        times relative to its start, the last one cut open; now and then one id is misheard"""
        segs, t = [], 0.3
        while t < 20.0 * n_chunks + 12:
            dur = float(rng.uniform(1.0, 6.0))
            segs.append((round(t / 0.02) * 0.02, round((t + dur) / 0.02) * 0.02, txt(int(rng.integers(2, 14)))))
            t += dur + (0.0 if rng.random() < 0.6 else float(rng.uniform(0.1, 1.5)))
        rows, start = [], 0.0
        for k in range(n_chunks):
            stride = FULL if n_chunks == 1 else FIRST if k == 0 else LAST if k == n_chunks - 1 else MID
            ids, tt = list(PROMPT), [0.0] * len(PROMPT)
            for s0, s1, words in segs:
                if s1 <= start or s0 >= start + 30.0:
                    continue
                lo = max(s0, start)
                ids.append(T(lo - start))
                tt.append(lo - start)
                m = len(words)
                for j, w in enumerate(words):
                    tw_ = s0 + (s1 - s0) * (j + 1) / (m + 1)
                    if start <= tw_ < start + 30.0:
                        ids.append(w if rng.random() > 0.03 else int(rng.integers(0, 50000)))
                        tt.append(round((tw_ - start) / 0.02) * 0.02)
                if s1 <= start + 30.0:
                    ids.append(T(s1 - start))
                    tt.append(s1 - start)
            rows.append((ids + [EOT], stride))
            tt.append(tt[-1])
            rows[-1] = (rows[-1][0], rows[-1][1], tt)
            start += 20.0
        return [(i, s) for i, s, _ in rows], [t for _, _, t in rows]

    for n_chunks in (1, 4, 9):
        rows, tt = simulate(n_chunks)
        put(f"batch_rec_{n_chunks}", rows, times=tt)

    # the reset: a chunk sets a start, gathers no text and nothing is pending, so HF forgets the start; without the rule the first
    # case closes (3.0, 26.0) at chunk 2's T(6) and the second closes (3.0, 28.0) with b instead of leaving (28.0, None) open
    put("reset_forgets_start", [(PROMPT + [T(3), EOT], (480000, 0, 0)), (PROMPT + [T(6)] + b + [T(8), EOT], LAST)])
    put("reset_forgets_start_strided", [(PROMPT + [T(3), T(27), EOT], FIRST), (PROMPT + [T(6)] + b + [T(8), EOT], LAST)])
    return c


def main():
    import transformers
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_chunked_ts_ref import KNOBS, seg_bits, segments_ref
    out = {"transformers_version": np.asarray(transformers.__version__)}
    names, want = [], {}
    for name, (rows, (tb, fs, tp, seg)) in cases().items():
        names.append(name)
        out[f"{name}_ids"] = np.asarray([t for ids, _, _ in rows for t in ids], np.int32)
        out[f"{name}_lens"] = np.asarray([len(ids) for ids, _, _ in rows], np.int32)
        out[f"{name}_strides"] = np.asarray([s for _, s, _ in rows], np.int32).reshape(-1, 3)
        out[f"{name}_times"] = np.concatenate([t for _, _, t in rows]).astype(np.float32)
        out[f"{name}_params"] = np.asarray([tb, fs, seg], np.int32)
        out[f"{name}_tp"] = np.asarray(tp, np.float64)
        for mode in ("segments", "word"):
            rec = hf_segments(rows, mode == "word", tb, fs, tp, seg)
            nan = float("nan")
            out[f"{name}_{mode}_seg_times"] = np.asarray([(nan if s is None else s, nan if e is None else e) for s, e, _, _ in rec], np.float64).reshape(-1, 2)
            ends = np.cumsum([len(i) for _, _, i, _ in rec]).astype(np.int32) if rec else np.zeros(0, np.int32)
            out[f"{name}_{mode}_seg_range"] = np.stack([ends - np.asarray([len(i) for _, _, i, _ in rec], np.int32), ends], 1).reshape(-1, 2).astype(np.int32)
            out[f"{name}_{mode}_ids"] = np.asarray([t for _, _, i, _ in rec for t in i], np.int32)
            if mode == "word":
                out[f"{name}_{mode}_pairs"] = np.asarray([p for _, _, _, ps in rec for p in ps], np.float64).reshape(-1, 2)
            segs = [dict({"timestamp": (s, e), "ids": i}, **({"token_timestamps": ps} if mode == "word" else {})) for s, e, i, ps in rec]
            want[name, mode] = (rows, dict(timestamp_begin=tb, first_special=fs, time_precision=tp, segment_size=seg), segs)
            got = segments_ref(rows, mode == "word", tb, fs, tp, seg)
            assert seg_bits(got) == seg_bits(segs), (name, mode)
            print(f"{name:32s} {mode:8s} {len(rec):3d} segments, {sum(len(i) for _, _, i, _ in rec):4d} ids")
    for case, mode, knob in KNOBS:  # every rule decides the case the fixture holds for it
        rows, par, segs = want[case, mode]
        assert seg_bits(segments_ref(rows, mode == "word", **par, **knob)) != seg_bits(segs), (case, mode, knob)
    assert [t for s in want["pair_out_of_order", "word"][2] for t in s["ids"]] != [t for s in want["pair_out_of_order", "segments"][2] for t in s["ids"]]
    out["names"] = np.asarray(names)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes;", len(names), "cases in two modes")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    main()
