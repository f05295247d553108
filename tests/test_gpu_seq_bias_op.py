"""Op-level tests (-m gpu) of sequence_bias / bad_words_ids: the logits + argmax (+ log-prob) launch on given hit state
(wm_op_logits_seq_bias) against float64, row isolation, and the hit state's bookkeeping (wm_op_seq_bias_hits: the init kernel and the
argmax launch's update) against the numpy reference of tests/test_seq_bias_ref.py, bit for bit.

Bound: the one tests/test_gpu_repeat_op.py uses for its processed logits (the per-logit bound of the launch, times max(p, 1/p) at a
penalised id) plus one fp32 rounding u·|z + bias| of the addition, scaled by the penalty like the rest."""
import numpy as np
import pytest

from test_gpu_decode_ops import DT_BF16, DT_F16, DT_F32, _call_logits, _ct, _decoder_like, _logits_ref, _lowest_argmax, hip  # noqa: F401
from test_gpu_repeat_op import P, _expect
from test_repeat_ref import bit_set
from test_seq_bias_ref import hit_state

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _state(B, N, r):
    """slot ids at columns 0, 31, 32, the last id, both sides of a logits-part boundary and random ones; per row a random subset on,
    some with a ban; id 32 stands for the id that carries a length-1 bias and a sequence bias (its slot holds the sum)."""
    part = 16 * _ct(N)
    sid = sorted({0, 31, 32, N - 1, min(part, N - 1) - 1, min(part, N - 1), 777 % N} | set(r.choice(N, 8, replace=False).tolist()))
    S = len(sid)
    bias = (r.standard_normal((B, S)) * 5).astype(np.float32)
    bias[:, sid.index(32)] = np.float32(2.5) + np.float32(-0.75)
    flags = np.zeros((B, S), np.int32)
    for b in range(B):
        on = r.random(S) < 0.7
        on[[sid.index(t) for t in (0, 31, 32, N - 1, min(part, N - 1) - 1, min(part, N - 1))]] = True
        flags[b] = on.astype(np.int32)
        flags[b, r.choice(S, 3, replace=False)] |= 2 * (r.random(3) < 0.7)
        flags[b] = np.where(flags[b] & 2, flags[b] | 1, flags[b])
    hit = np.stack([bit_set([sid[k] for k in range(S) if flags[b, k] & 1], N) for b in range(B)])
    return np.asarray(sid, np.int32), bias, flags, hit


@pytest.mark.parametrize("B,N", [(3, 1000), (17, 51865), (33, 1000)])
@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("dt", [DT_F32, DT_BF16, DT_F16])
def test_processed_logits_vs_float64(hip, dt, K, B, N):
    r = np.random.default_rng(31 * K + 7 * B + N + dt)
    x, g, b, emb = _decoder_like(r, B, K, N, dt)
    plain, pids = _call_logits(x, g, b, emb, dt)
    sid, bias, flags, hit = _state(B, N, r)
    # seen: half of the slots' ids (bias then penalty) and a few others; ban: two ids without a slot
    seen = [sorted(set(sid[::2].tolist()) | {5, N // 3}) for _ in range(B)]
    nb = [t for t in (9, N // 5) if t not in sid]
    sw = np.stack([bit_set(s, N) for s in seen])
    bw = np.stack([bit_set(nb, N) for _ in range(B)])
    mask = np.zeros(N, np.float32)
    mask[[3, N // 2]] = -np.inf
    kw = dict(mask=mask, seen=sw, ban=bw, penalty=P, hit=hit, slot_id=sid, slot_bias=bias, slot_flags=flags)
    logits, ids, lp = _call_logits(x, g, b, emb, dt, return_logprobs=True, **kw)
    l2, i2 = _call_logits(x, g, b, emb, dt, **kw)  # the instantiation without log-probs
    np.testing.assert_array_equal(l2, logits)
    np.testing.assert_array_equal(i2, ids)
    ref, bound = _logits_ref(x, g, b, emb, dt)
    for bb in range(B):
        on = (flags[bb] & 1) != 0
        banned = set(sid[(flags[bb] & 2) != 0].tolist()) | set(nb)
        r1, b1 = ref[bb:bb + 1].copy(), bound[bb:bb + 1].copy()
        r1[0, sid[on]] += bias[bb, on].astype(np.float64)
        b1[0, sid[on]] += U * np.abs(r1[0, sid[on]])
        want, bnd = _expect(r1, b1, [seen[bb]], [sorted(banned)], P)
        k = np.asarray(sorted(banned))
        assert (logits[bb, k] == -np.inf).all() and ids[bb] not in banned
        keep = np.setdiff1d(np.arange(N), k)
        err = np.abs(logits[bb, keep] - want[0, keep])
        s = np.asarray(seen[bb])
        near0 = np.isin(keep, s[np.abs(r1[0, s]) <= b1[0, s]])  # the penalty's sign test at a logit within its bound of 0
        other = np.where(r1[0, keep] < 0, r1[0, keep] / P, r1[0, keep] * P)
        err = np.where(near0, np.minimum(err, np.abs(logits[bb, keep] - other)), err)
        ratio = err / bnd[0, keep]
        assert ratio.max() <= 1.0, (bb, int(keep[np.argmax(ratio)]), ratio.max())
        same = np.setdiff1d(keep, np.union1d(seen[bb], sid[on]))
        np.testing.assert_array_equal(logits[bb, same], plain[bb, same])
        off = sid[~on]
        off = off[~np.isin(off, seen[bb])]
        np.testing.assert_array_equal(logits[bb, off], plain[bb, off])  # a slot that is off adds nothing
    np.testing.assert_array_equal(ids, _lowest_argmax(logits + mask))
    assert np.isfinite(lp).all()


@pytest.mark.parametrize("dt,K,B", [(DT_F32, 384, 3), (DT_BF16, 384, 3), (DT_F32, 128, 33), (DT_F16, 128, 17)])
def test_only_the_rows_own_hits_count(hip, dt, K, B):
    """Row 1 alone has hits: every other row equals the launch with null pointers bit for bit, logits, ids and log-probs."""
    N = 51865
    r = np.random.default_rng(K + B + dt)
    x, g, b, emb = _decoder_like(r, B, K, N, dt)
    plain, pids, plp = _call_logits(x, g, b, emb, dt, return_logprobs=True)
    top = int(pids[1])
    sid = np.asarray(sorted({0, 777, top, N - 1}), np.int32)
    bias, flags = np.full((B, sid.size), 1e6, np.float32), np.zeros((B, sid.size), np.int32)  # (stale slot values of the other rows)
    flags[1] = 1
    flags[1, sid.tolist().index(top)] = 3
    bias[1] = 4.0
    hit = np.zeros((B, (N + 31) // 32), np.uint32)
    hit[1] = bit_set(sid.tolist(), N)
    z = np.zeros_like(hit)
    logits, ids, lp = _call_logits(x, g, b, emb, dt, seen=z, ban=z, penalty=1.0, hit=hit, slot_id=sid, slot_bias=bias, slot_flags=flags,
                                   return_logprobs=True)
    others = [i for i in range(B) if i != 1]
    np.testing.assert_array_equal(logits[others], plain[others])
    np.testing.assert_array_equal(ids[others], pids[others])
    np.testing.assert_array_equal(lp[others], plp[others])
    assert ids[1] != top and logits[1, top] == -np.inf
    for t in (0, 777, N - 1):
        if t != top:
            assert logits[1, t] == np.float32(plain[1, t] + np.float32(4.0))
    # no hit anywhere: the SB instantiation computes what the plain one does
    l0, i0, lp0 = _call_logits(x, g, b, emb, dt, seen=z, ban=z, penalty=1.0, hit=z, slot_id=sid, slot_bias=bias, slot_flags=flags,
                               return_logprobs=True)
    np.testing.assert_array_equal(l0, plain)
    np.testing.assert_array_equal(i0, pids)
    np.testing.assert_array_equal(lp0, plp)


@pytest.mark.parametrize("vocab", [1000, 51865])
def test_hit_state_follows_the_history(hip, vocab):
    """Histories of 447, 63 and 30 ids over a small alphabet, prompts of 1, 5 and 17 ids: slots (on, ban, the fp32 sum) and bits equal
    the numpy reference after the init and after every step, bit for bit.  The table holds a sequence that spans the prompt /
    generated boundary of row 1, two sequences with overlapping prefixes, sequences that end in the same id with biases whose sum
    depends on the order, a sequence equal to row 2's whole history at one step, a length-1 bias on an id that also ends longer
    sequences, an [eot] bad word, and ids at the vocabulary's and the words' edges."""
    from whisper_mojo_amd import whisper_tensor as wt
    r = np.random.default_rng(vocab)
    alphabet = np.array([0, 31, 32, 33, vocab - 26, vocab - 1])
    plen, nids = [1, 5, 17], [447, 63, 30]
    tok = np.zeros((3, 447), np.int32)
    for b in range(3):
        tok[b, :nids[b]] = r.choice(alphabet[:3 + b + (b > 0)], nids[b])
    A = [int(a) for a in alphabet]
    sb = {(A[0], A[1], A[2]): 1e8, (A[1], A[2]): -1e8, (A[2],): 1.0, (A[1], A[1], A[2]): 0.37,
          tuple(int(t) for t in tok[1, 3:7]): 2.0,                # spans row 1's prompt / generated boundary (prompt = 5 ids)
          tuple(int(t) for t in tok[2, :20]): -3.0,               # row 2's whole history after three steps
          tuple(int(t) for t in tok[2, :21]): -4.0,               # one id longer than the history it would need: HF's `continue`
          (A[0], A[0]): float("-inf"), (A[5],): 0.5, (A[0], A[5]): 0.25, (A[1], A[0], A[5]): 0.125}
    bad = [[A[0], A[1]], [A[1], A[0], A[1]], [A[4]], [7], [A[2], A[5]]]
    eot, steps = 7, 446
    sid, hit, bias, flags = wt.seq_bias_hits(tok, plen, nids, vocab, sb, bad, steps, eot=eot)
    changed = 0
    for b in range(3):
        prev = None
        for s in range(steps + 1):
            L = min(plen[b] + s, nids[b])
            wsid, wbias, wflags, whit = hit_state(tok[b, :L].tolist(), sb, bad, vocab, eot)
            if s == 0 and b == 0:
                np.testing.assert_array_equal(sid, wsid)
            assert flags[s, b].tolist() == wflags.tolist(), (b, s)
            np.testing.assert_array_equal(bias[s, b].view(np.uint32), wbias.view(np.uint32), err_msg=f"row {b} step {s}")
            np.testing.assert_array_equal(hit[s, b], whit, err_msg=f"row {b} step {s}")
            changed += prev is not None and prev != wflags.tolist()
            prev = wflags.tolist()
    assert changed > 50  # slots do go on and off
