"""CPU-only: a numpy restatement of HF WhisperTimeStampLogitsProcessor's rules 1-4 (which ids may follow a generated history), checked
against the oracle's processor and the HF-made rule table of tests/golden/micro_timestamps.npz, plus the case generators and numpy
expectations of the op tests in tests/test_gpu_ts_states_op.py and tests/test_gpu_pass_control_op.py.

The rules, on the ids generated so far (`seq`, behind the prompt), with tb = timestamp_begin:
  1. nothing generated yet: a timestamp, at most tb + max_initial when max_initial is given;
  2. the last id is a timestamp and so is the one before (or there is none before): no timestamp;
     the last id is a timestamp and the one before is not: no id below eos;
  3. timestamps never decrease: none below the last one emitted — and not that one either, unless it opened a pair just now (rule 2's
     second case);
  4. <|notimestamps|> never (the kernels take that one from the suppress mask, so `admissible` applies it only when asked).
Rule 5 (a timestamp is forced when the timestamps' probability mass exceeds every text id's) is the decision, not the set: it is
tests/test_gpu_decode_ops.py's _ts_decision."""
import itertools

import numpy as np

from conftest import golden


def admissible(seq, vocab, tb, eos, max_initial=None, no_timestamps=None):
    """Boolean [vocab]: the ids rules 1-4 leave after the generated ids `seq`."""
    ok = np.ones(vocab, bool)
    seq = [int(t) for t in seq]
    if no_timestamps is not None:
        ok[no_timestamps] = False
    last = len(seq) >= 1 and seq[-1] >= tb
    pen = len(seq) < 2 or seq[-2] >= tb
    if last:
        if pen:
            ok[tb:] = False
        else:
            ok[:eos] = False
    ts = [t for t in seq if t >= tb]
    if ts:
        ok[tb:ts[-1] if (last and not pen) else ts[-1] + 1] = False
    if not seq:
        ok[:tb] = False
        if max_initial is not None:
            ok[tb + max_initial + 1:] = False
    return ok


def history_fields(seq, tb):
    """(n_gen, last_ts, pen_ts, t_last) of TsState after the generated ids `seq`."""
    seq = [int(t) for t in seq]
    ts = [t for t in seq if t >= tb]
    return (len(seq), int(len(seq) >= 1 and seq[-1] >= tb), int(len(seq) < 2 or seq[-2] >= tb), ts[-1] if ts else -1)


def range_ids(state, vocab):
    """The id set [text_lo, text_hi) ∪ [ts_lo, ts_hi) of one TsState (eight ints) as a boolean [vocab]: an empty range has many encodings."""
    ok = np.zeros(vocab, bool)
    for lo, hi in ((state[4], state[5]), (state[6], state[7])):
        assert 0 <= lo <= vocab and hi <= vocab, state
        if hi > lo:
            ok[lo:hi] = True
    return ok


def enumerate_histories(vocab, tb, eos, max_initial, depth):
    """Every history of `depth` generated ids in which each id was admissible at its step, in lexicographic order."""
    level = [()]
    for _ in range(depth):
        level = [h + (int(t),) for h in level for t in np.flatnonzero(admissible(h, vocab, tb, eos, max_initial))]
    return level


def enumeration_depth(vocab, tb, eos, max_initial, lo=1000, hi=4096):
    """The depth whose leaf count lies in [lo, hi], with the leaves."""
    for depth in range(1, 12):
        leaves = enumerate_histories(vocab, tb, eos, max_initial, depth)
        if len(leaves) >= lo:
            assert len(leaves) <= hi, (depth, len(leaves))
            return depth, leaves
    raise AssertionError("no depth reaches the row count")


SMALL = dict(vocab=12, tb=8, eos=5)  # text ids 0-4, specials 5-7, four timestamps
# Histories no admissible walk reaches (after the first generated timestamp rule 2 refuses every timestamp): the state machine still has
# to follow them — the fused argmax takes whatever id the logits stage hands it.  HF's processor is defined on them too (the fixture's
# table has [tb, tb]).
OFF_POLICY = [(8, 8), (8, 9), (9, 9, 9), (8, 8, 3, 8), (11, 11), (10, 11, 11, 11), (2, 3), (3,), (2, 9, 9, 9), (9, 8), (11, 2, 8, 8)]


def table_rows(prompts, histories, stride=None):
    """tokens [B, stride], prompt_len [B], n_ids [B] of a replay: row b = prompts[b] + histories[b]."""
    B = len(histories)
    stride = stride or max(len(p) + len(h) for p, h in zip(prompts, histories))
    tok = np.zeros((B, stride), np.int32)
    for b, (p, h) in enumerate(zip(prompts, histories)):
        tok[b, :len(p) + len(h)] = list(p) + list(h)
    return tok, np.array([len(p) for p in prompts], np.int32), np.array([len(p) + len(h) for p, h in zip(prompts, histories)], np.int32)


def ragged_prompts(B, vocab, lo=1, hi=5):
    """Row b's prompt: (b % (hi - lo + 1)) + lo ids that name the row."""
    return [[(b + 3 * i) % vocab for i in range(lo + b % (hi - lo + 1))] for b in range(B)]


# ---- numpy expectations of the pass-control kernels (tests/test_gpu_pass_control_op.py) ---------------------------------------

def init_state(vocab, tb, eos, max_initial):
    """TsState (eight ints) the init kernels write: nothing generated, the first id a timestamp."""
    hi = vocab if max_initial is None or max_initial < 0 else min(vocab, tb + max_initial + 1)
    return np.array([0, 0, 1, -1, 0, 0, tb, hi], np.int32)


def init_tokens_expect(bufs, B, out_stride, prompt=None, table=None, lens=None, Lmax=None, ts=None):
    """What init_tokens_kernel (prompt) / init_tokens_rows_kernel (table [B, stride], lens, Lmax) leave in the caller's buffers: a dict
    of the same arrays, written where the kernel writes and nowhere else.  ts = (vocab, tb, eos, max_initial) with a ts_state buffer."""
    out = {k: (None if v is None else v.copy()) for k, v in bufs.items()}
    rows = table is not None
    for b in range(B):
        ids = list(table[b, :lens[b]]) if rows else list(prompt)
        out["out_tokens"][b, :len(ids)] = ids
        out["n_tokens"][b] = len(ids)
        out["finished"][b] = 0
        if out.get("logprobs") is not None:
            out["logprobs"][b, :] = 0
            out["lp_sum"][b] = 0
        if rows:
            pad = Lmax - lens[b]
            out["key_lo"][b] = pad
            out["tok_rows"][:Lmax, b] = [ids[0]] * pad + ids
            out["pos_rows"][:Lmax, b] = [0] * pad + list(range(len(ids)))
        elif out.get("tok_rows") is not None:
            out["tok_rows"][:len(ids), b] = ids
            out["pos_rows"][:len(ids), b] = range(len(ids))
        if out.get("ts_state") is not None:
            out["ts_state"][b] = init_state(*ts)
    out["ctl"][:2] = 0  # len, n_finished; the two pad words stay
    return out


def pack_tokens_expect(dst, out_tokens, n_tokens, rows, rows_cap, stride):
    """pack_tokens_kernel: dst[r] = [n, ids zero-padded to stride], n = min(n_tokens[r], stride); rows in [rows, rows_cap) zeroed."""
    want = dst.copy()
    for r in range(rows_cap):
        n = min(int(n_tokens[r]), stride) if r < rows else 0
        want[r, 0] = n
        want[r, 1:1 + stride] = 0
        if n:
            want[r, 1:1 + n] = out_tokens[r, :n]
    return want


def rows_copy_expect(out, rows, dst):
    """score_collect_kernel: out[dst[r]] = rows[r] where dst[r] >= 0 (dst None: the plain copy of no_speech_capture_kernel)."""
    want = out.copy()
    for r in range(rows.shape[0]):
        o = r if dst is None else int(dst[r])
        if o >= 0:
            want[o] = rows[r]
    return want


def mel_image_expect(mel, Cp, rounded):
    """mel_transpose_pad_kernel: [B, C, L] -> [B, L + 2, Cp], row t + 1 = frame t (`rounded` = the mel in the operand type), rows 0 and
    L + 1 and channels >= C zero."""
    B, C, L = mel.shape
    want = np.zeros((B, L + 2, Cp), np.float32)
    want[:, 1:L + 1, :C] = np.transpose(rounded, (0, 2, 1))
    return want


# ---- the reference checks itself ---------------------------------------------------------------------------------------------

def _fixture():
    g = golden("micro_timestamps")
    return g, int(g["timestamp_begin"]), int(g["no_timestamps"]), int(g["eos"]), int(g["max_initial"])


def test_admissible_matches_hf_rule_table():
    """HF's own processor output: where rule 5 did not fire the finite ids are the admissible set; where it did, the finite ids are the
    admissible timestamps."""
    g, tb, no_ts, eos, max_init = _fixture()
    V = g["rows"].shape[2]
    free = 0
    for h, hist in enumerate(g["histories"]):
        seq = [int(t) for t in hist if t >= 0]
        ok = admissible(seq, V, tb, eos, max_init, no_ts)
        for r in range(g["rows"].shape[1]):
            fin = ~np.isneginf(g["processed"][h, r])
            if fin[:tb].any():
                assert np.array_equal(fin, ok), (seq, r)
                free += 1
            else:
                assert np.array_equal(fin[tb:], ok[tb:]), (seq, r)
    assert free >= len(g["histories"]) // 2  # the table does show the text side


def test_admissible_matches_the_oracle():
    """The oracle's processor on scores whose text side dominates (rule 5 cannot fire: every timestamp is 50 below every text id, and
    there are at most a few thousand of them), over the fixture's histories, the small vocabulary's whole enumeration with its
    off-policy rows, and Whisper's real layout."""
    from oracle import oracle
    g, tb, no_ts, eos, max_init = _fixture()
    cases = [(1000, tb, eos, max_init, no_ts, [[int(t) for t in h if t >= 0] for h in g["histories"]])]
    V, TB, EOS = SMALL["vocab"], SMALL["tb"], SMALL["eos"]
    for mi in (None, 0, 1, 3, 50):
        for e in (EOS, TB):
            hs = [h[:k] for h in enumerate_histories(V, TB, e, mi, 3) + OFF_POLICY for k in range(len(h) + 1)]
            cases.append((V, TB, e, mi, None, sorted(set(hs))))
    cases.append((51865, 50364, 50257, 50, 50363, [[], [50364], [50414, 7], [50364, 7, 51864], [50364, 7, 51864, 51864], [50364, 7, 51864, 51864, 9],
                                                   [50364, 50364], [50400, 1, 2, 50401], [51864]]))
    for V, TB, e, mi, nts, hists in cases:
        scores = np.zeros(V, np.float32)
        scores[TB:] = -50.0
        for seq in hists:
            got = oracle.timestamp_rules(scores, seq, TB, -1 if nts is None else nts, e, mi)
            ok = admissible(seq, V, TB, e, mi, nts)
            if not ok[:TB].any():  # no text id left: rule 5 has nothing to compare, the timestamps stand
                assert np.array_equal(~np.isneginf(got)[TB:], ok[TB:]), (V, e, mi, seq)
            else:
                assert np.array_equal(~np.isneginf(got), ok), (V, e, mi, seq)


def test_enumeration_holds_the_named_cases():
    """The exhaustive walk of the small vocabulary: depth and row count as the GPU test's docstring states them, and the states the
    issue names are among its prefixes (or, where no admissible walk reaches them, among the off-policy rows)."""
    V, tb, eos = SMALL["vocab"], SMALL["tb"], SMALL["eos"]
    depth, leaves = enumeration_depth(V, tb, eos, None)
    assert (depth, len(leaves)) == (ENUM_DEPTH, ENUM_ROWS)
    found = named_cases(leaves + OFF_POLICY, V, tb, eos, None)
    assert all(found.values()), found
    # after the first generated timestamp every timestamp is refused: "two timestamps first" can only be forced
    assert not any(h[0] >= tb and h[1] >= tb for h in leaves) and any(len(h) >= 2 and h[0] >= tb and h[1] >= tb for h in OFF_POLICY)
    # the other settings walk the same depth; the smallest walk (max_initial = 0: one first id) still has hundreds of rows
    counts = {(mi, e): len(enumerate_histories(V, tb, e, mi, depth)) for mi in (None, 0, 1, 3, 50) for e in (eos, tb)}
    assert min(counts.values()) == counts[(0, tb)] == 752 and max(counts.values()) == ENUM_ROWS, counts


ENUM_DEPTH, ENUM_ROWS = 4, 2656  # enumeration_depth(12, 8, 5, None): depth 3 has 304 rows, depth 5 has 23136


def named_cases(histories, vocab, tb, eos, max_initial):
    """Which of the issue's named states occur among the prefixes of `histories`."""
    found = dict(closed_pair_same_refused=False, open_pair_same_allowed=False, last_id_empties_range=False, two_timestamps_first=False)
    for h in histories:
        for k in range(1, len(h) + 1):
            p = h[:k]
            _, last, pen, t_last = history_fields(p, tb)
            ok = admissible(p, vocab, tb, eos, max_initial)
            if k >= 2 and p[-1] >= tb and p[-2] == p[-1] and not ok[p[-1]]:
                found["closed_pair_same_refused"] = True
            if last and not pen and ok[t_last]:
                found["open_pair_same_allowed"] = True
            if t_last == vocab - 1 and not ok[tb:].any() and not (last and pen and t_last != vocab - 1):
                found["last_id_empties_range"] = True
            if k == 2 and p[0] >= tb and p[1] >= tb:
                found["two_timestamps_first"] = True
    return found


def test_pass_control_expectations_on_hand_cases():
    """The numpy expectations of the pass-control kernels on cases small enough to read."""
    s = -7
    bufs = dict(out_tokens=np.full((2, 6), s, np.int32), n_tokens=np.full(2, s, np.int32), finished=np.full(2, s, np.int32),
                ctl=np.full(4, s, np.int32), tok_rows=np.full((4, 2), s, np.int32), pos_rows=np.full((4, 2), s, np.int32),
                key_lo=np.full(2, s, np.int32), ts_state=np.full((2, 8), s, np.int32), logprobs=None, lp_sum=None)
    table = np.array([[5, 6, 7, 0], [9, 0, 0, 0]], np.int32)
    w = init_tokens_expect(bufs, 2, 6, table=table, lens=[3, 1], Lmax=3, ts=(12, 8, 5, 1))
    assert w["out_tokens"].tolist() == [[5, 6, 7, s, s, s], [9, s, s, s, s, s]] and w["n_tokens"].tolist() == [3, 1]
    assert w["tok_rows"].tolist() == [[5, 9], [6, 9], [7, 9], [s, s]] and w["pos_rows"].tolist() == [[0, 0], [1, 0], [2, 0], [s, s]]
    assert w["key_lo"].tolist() == [0, 2] and w["ctl"].tolist() == [0, 0, s, s]
    assert w["ts_state"][0].tolist() == [0, 0, 1, -1, 0, 0, 8, 10]
    assert init_state(12, 8, 5, 50).tolist() == [0, 0, 1, -1, 0, 0, 8, 12] and init_state(12, 8, 5, None)[7] == 12
    d = np.full((3, 4), s, np.int32)
    got = pack_tokens_expect(d, np.array([[1, 2, 3, 4, 5], [6, 7, 8, 9, 10]], np.int32), [2, 5], 2, 3, 3)
    assert got.tolist() == [[2, 1, 2, 0], [3, 6, 7, 8], [0, 0, 0, 0]]
    o = rows_copy_expect(np.zeros((3, 2)), np.array([[1., 1.], [2., 2.]]), [2, -1])
    assert o.tolist() == [[0, 0], [0, 0], [1, 1]]
    m = np.arange(6, dtype=np.float32).reshape(1, 2, 3)
    assert mel_image_expect(m, 4, m)[0].tolist() == [[0, 0, 0, 0], [0, 3, 0, 0], [1, 4, 0, 0], [2, 5, 0, 0], [0, 0, 0, 0]]


def test_new_hooks_are_bound():
    from whisper_mojo_amd import _lib
    for name in ("wm_op_ts_states", "wm_op_init_tokens", "wm_op_set_rows_step", "wm_op_set_step", "wm_op_pack_tokens", "wm_op_dec_embed",
                 "wm_op_rows_copy", "wm_op_mel_transpose_pad"):
        assert name in _lib.SYMBOLS


if __name__ == "__main__":
    print("depth, rows:", enumeration_depth(SMALL["vocab"], SMALL["tb"], SMALL["eos"], None)[0], ENUM_ROWS)
    for mi, e in itertools.product((None, 0, 1, 3, 50), (5, 8)):
        print(f"max_initial {mi} eos {e}:", [len(enumerate_histories(SMALL["vocab"], SMALL["tb"], e, mi, d)) for d in (3, 4, 5)])
