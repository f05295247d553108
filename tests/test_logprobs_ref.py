"""CPU tests of the log-probability rule: a numpy float64 restatement of what wm_transcribe_lp computes — the suppress
masks, the timestamp rules' admissible ranges (the arithmetic of ts_next_ranges in wm_kernels.h), the forced-timestamp decision and
the normaliser of each branch — applied to the RAW logits stored in tests/golden/logprobs_micro_hf.npz reproduces HF's ids and
log_softmax(processed scores)[id] to 1e-5 (HF fp32 log_softmax against float64), and _retrieve_avg_logprobs to the same.  The fixture
must contain every normaliser branch.  Plus the host wrappers' shape checks, which need no library."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def lse(v):
    v = v[v > -np.inf]
    if v.size == 0:
        return -np.inf
    m = v.max()
    return m + np.log(np.exp(v - m).sum())


def restate_logprobs(raw, n_prompt, sup, bsup, ts, tb, eos, no_ts, max_init):
    """raw [steps, V] -> (ids, logprobs, branches): greedy ids by the library's rule, the log-prob of each, the normaliser branch"""
    V = raw.shape[1]
    ids, lps, branches = [], [], []
    n_gen, last_ts, pen_ts, t_last = 0, 0, 1, -1
    for step in range(raw.shape[0]):
        s = raw[step].astype(np.float64).copy()
        s[list(sup)] = -np.inf
        if step == 0:
            s[list(bsup)] = -np.inf
        if not ts:
            pick = int(np.argmax(s))
            lps.append(s[pick] - lse(s))
            branches.append("off")
            ids.append(pick)
            continue
        s[no_ts] = -np.inf
        text_lo, text_hi, ts_lo, ts_hi = 0, tb, tb, V  # ts_next_ranges
        if n_gen == 0:
            text_hi = 0
            if max_init >= 0:
                ts_hi = min(ts_hi, tb + max_init + 1)
        else:
            if last_ts:
                if pen_ts:
                    ts_hi = ts_lo
                else:
                    text_lo = eos
            if t_last >= 0:
                ts_lo = max(ts_lo, t_last if (last_ts and not pen_ts) else t_last + 1)
        text, tss = s[text_lo:text_hi], s[ts_lo:max(ts_hi, ts_lo)]
        best = text.max() if text.size else -np.inf
        forced = lse(tss) > -np.inf and (best == -np.inf or lse(tss) > best)
        if forced:
            pick = ts_lo + int(np.argmax(tss))
            lps.append(s[pick] - lse(tss))
        else:
            pick = text_lo + int(np.argmax(text))
            lps.append(s[pick] - lse(np.concatenate([text, tss])))
        branches.append("forced" if forced else "mixed")
        ids.append(pick)
        is_ts = pick >= tb
        pen_ts = 1 if n_gen + 1 < 2 else last_ts
        last_ts = int(is_ts)
        n_gen += 1
        if is_ts:
            t_last = pick
    return ids, np.asarray(lps), branches


def test_restatement_reproduces_hf_fixture():
    z = np.load(os.path.join(GOLDEN, "logprobs_micro_hf.npz"))
    seen, worst = set(), 0.0
    for i in range(int(z["n_rows"])):
        k = f"r{i}_"
        prompt, want = z[k + "prompt"], z[k + "ids"]
        raw = z[k + "raw"]
        ids, lps, br = restate_logprobs(raw, len(prompt), z["suppress"], z["begin_suppress"], int(z[k + "ts"]), int(z["timestamp_begin"]),
                                        int(z["eos"]), int(z["no_ts"]), int(z["max_init"]))
        assert ids == want[len(prompt):].tolist(), i
        err = np.abs(lps - z[k + "logprobs"].astype(np.float64)).max()
        aerr = abs(lps.mean() - float(z[k + "avg_logprob"]))
        worst = max(worst, err, aerr)
        assert err <= 1e-5 and aerr <= 1e-5, (i, err, aerr)
        assert (z[k + "logprobs"] <= 0).all()
        seen |= set(br)
    print(f"worst |restatement - HF| {worst:.2e}; branches {sorted(seen)}")
    assert seen == {"forced", "mixed", "off"}


def test_tiny_fixture_has_the_cases():
    z = np.load(os.path.join(GOLDEN, "logprobs_tiny_hf.npz"))
    cases = [str(z[f"r{i}_case"]) for i in range(int(z["n_rows"]))]
    assert {"shared", "off", "rows"} <= set(cases)
    tb = int(z["timestamp_begin"])
    for i, c in enumerate(cases):
        ids, p, lps = z[f"r{i}_ids"], z[f"r{i}_prompt"], z[f"r{i}_logprobs"]
        assert len(ids) - len(p) == len(lps)
        assert abs(float(lps.astype(np.float64).mean()) - float(z[f"r{i}_avg_logprob"])) <= 1e-5
        gen = ids[len(p):]
        if c != "off":  # a forced timestamp (the first id) and text ids: both branches of the rules
            assert gen[0] >= tb and (gen < tb).any()


def test_host_wrappers_refuse_bad_shapes():
    from whisper_mojo_amd import whisper_tensor as wt
    x = np.zeros((2, 128), np.float32)
    with pytest.raises(ValueError):
        wt.logits_argmax(x, np.ones(64), np.zeros(128), np.zeros((100, 128)), return_logprobs=True)
    with pytest.raises(ValueError):
        wt.logits_argmax(x, np.ones(128), np.zeros(128), np.zeros((100, 64)), return_logprobs=True)
    with pytest.raises(ValueError):
        wt.logits_argmax(x, np.ones(128), np.zeros(128), np.zeros((100, 128)), mask=np.zeros(99), return_logprobs=True)
    with pytest.raises(ValueError):
        wt.logits_argmax(x, np.ones(128), np.zeros(128), np.zeros((100, 128)), ranges=np.zeros((3, 4)), timestamp_begin=50, return_logprobs=True)
    from whisper_mojo_amd.whisper import Whisper
    with pytest.raises(ValueError):
        Whisper._prompt_rows([[1, 2], [3]], 3)
