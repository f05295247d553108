"""Op-level tests (-m gpu) of the repetition processors: the logits + argmax (+ log-prob) launch on given sets
(wm_op_logits_processed) against float64, row isolation against the launch without the sets, and the sets' bookkeeping
(wm_op_repeat_sets: the init kernel and the argmax launch's update) against the numpy reference of tests/test_repeat_ref.py.

Bounds: the per-logit bound of tests/test_gpu_decode_ops.py (_logits_ref) for the same launch, times max(p, 1/p) at a penalised id
(the penalty scales the logit's error by p or 1/p); banned ids are exactly -inf.  Log-probs: the bound of tests/test_gpu_logits_lp.py
(_lp_ref) on the processed row, a banned id being one more masked candidate."""
import numpy as np
import pytest

from test_gpu_decode_ops import DT_BF16, DT_F16, DT_F32, _call_logits, _ct, _decoder_like, _logits_ref, _lowest_argmax, hip  # noqa: F401
from test_gpu_logits_lp import _lp_ref
from test_repeat_ref import banned_ids, bit_set, set_ids

pytestmark = pytest.mark.gpu

P = 1.3


def _sets(B, N, plain, r):
    """Per row: ids whose bits matter — first and last column of a word, the last valid id, a column-tile edge (15 | 16), a part
    edge, the row's unprocessed arg-max and its runner-up — dealt between `seen` and `ban` (some in both), plus random ones."""
    part = 16 * _ct(N)
    seen, ban = [], []
    for b in range(B):
        order = np.argsort(-plain[b], kind="stable")
        top, second = int(order[0]), int(order[1])
        edge = [0, 31, 32, 63, N - 1, 15, 16, min(part, N - 1) - 1, min(part, N - 1), (N - 1) // 32 * 32]
        rnd = r.choice(N, 12, replace=False).tolist()
        s = set(edge[0::2] + rnd[:6]) | ({top} if b % 3 != 2 else {second})
        k = set(edge[1::2] + rnd[4:10]) | ({top} if b % 3 == 0 else set()) | ({second} if b % 3 == 1 else set())
        s |= {3, N // 2}  # the masked ids (the callers mask 3 and N // 2): a penalised and a banned id under the mask
        k |= {N // 2}
        seen.append(sorted(s))
        ban.append(sorted(k))
    return seen, ban


def _expect(ref, bound, seen, ban, p):
    """float64 processed logits and their bound"""
    ref, bound = ref.copy(), bound.copy()
    for b in range(ref.shape[0]):
        s = np.asarray(seen[b], np.int64)
        neg = ref[b, s] < 0
        ref[b, s] = np.where(neg, ref[b, s] * p, ref[b, s] / p)
        bound[b, s] *= max(p, 1 / p)
        ref[b, ban[b]] = -np.inf
    return ref, bound


@pytest.mark.parametrize("B,N", [(1, 1000), (17, 51865), (33, 1000), (33, 51865)])
@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("dt", [DT_F32, DT_BF16, DT_F16])
def test_processed_logits_vs_float64(hip, dt, K, B, N):
    r = np.random.default_rng(17 * K + 5 * B + N + dt)
    x, g, b, emb = _decoder_like(r, B, K, N, dt)
    plain, pids = _call_logits(x, g, b, emb, dt)
    seen, ban = _sets(B, N, plain, r)
    sw = np.stack([bit_set(s, N) for s in seen])
    bw = np.stack([bit_set(s, N) for s in ban])
    mask = np.zeros(N, np.float32)
    mask[[3, N // 2]] = -np.inf
    logits, ids, lp = _call_logits(x, g, b, emb, dt, mask=mask, seen=sw, ban=bw, penalty=P, return_logprobs=True)
    l2, i2 = _call_logits(x, g, b, emb, dt, mask=mask, seen=sw, ban=bw, penalty=P)  # the instantiation without log-probs
    np.testing.assert_array_equal(l2, logits)
    np.testing.assert_array_equal(i2, ids)
    ref, bound = _logits_ref(x, g, b, emb, dt)
    want, bnd = _expect(ref, bound, seen, ban, P)
    for bb in range(B):
        k = np.asarray(ban[bb])
        assert (logits[bb, k] == -np.inf).all()
        assert ids[bb] not in ban[bb]
        keep = np.setdiff1d(np.arange(N), k)
        err = np.abs(logits[bb, keep] - want[bb, keep])
        # the penalty's sign test reads the kernel's own fp32 logit (HF's reads its own): a logit within its bound of 0 may take
        # the other branch — there the nearer of z·p and z/p counts
        s = np.asarray(seen[bb])
        near0 = np.isin(keep, s[np.abs(ref[bb, s]) <= bound[bb, s]])
        other = np.where(ref[bb, keep] < 0, ref[bb, keep] / P, ref[bb, keep] * P)
        err = np.where(near0, np.minimum(err, np.abs(logits[bb, keep] - other)), err)
        ratio = err / bnd[bb, keep]
        assert ratio.max() <= 1.0, (bb, int(keep[np.argmax(ratio)]), ratio.max())
        # untouched columns are the plain launch's, bit for bit
        same = np.setdiff1d(keep, seen[bb])
        np.testing.assert_array_equal(logits[bb, same], plain[bb, same])
    # arg-max: exact on the kernel's own processed logits under the mask, and within one bound of the float64 maximum
    cand = logits + mask
    np.testing.assert_array_equal(ids, _lowest_argmax(cand))
    w64 = want + mask
    sel = np.arange(B)
    assert (w64[sel, ids] >= w64.max(1) - bnd[sel, ids]).all()
    # log-probs: float64 log-sum-exp over the processed values the mask leaves
    for bb in range(B):
        m = mask.copy()
        m[ban[bb]] = -np.inf
        fin = np.where(np.isfinite(want[bb]), want[bb], 0.0)[None]
        w, e = _lp_ref(fin, bnd[bb:bb + 1], m, None, ids[bb:bb + 1], 0, N)
        assert np.isfinite(lp[bb]) and abs(lp[bb] - w[0]) <= e[0], (bb, lp[bb], w[0], e[0])


@pytest.mark.parametrize("dt,K,B", [(DT_F32, 384, 3), (DT_BF16, 384, 3), (DT_F32, 128, 33), (DT_F16, 128, 17)])
def test_only_the_rows_own_sets_count(hip, dt, K, B):
    """Row 1 alone has sets: every other row equals the launch with null pointers bit for bit, logits, ids and log-probs."""
    N = 51865
    r = np.random.default_rng(K + B + dt)
    x, g, b, emb = _decoder_like(r, B, K, N, dt)
    plain, pids, plp = _call_logits(x, g, b, emb, dt, return_logprobs=True)
    sw, bw = np.zeros((B, (N + 31) // 32), np.uint32), np.zeros((B, (N + 31) // 32), np.uint32)
    top = int(pids[1])
    sw[1] = bit_set([0, 31, 777, N - 1], N)
    bw[1] = bit_set([top, 32, N - 2], N)
    logits, ids, lp = _call_logits(x, g, b, emb, dt, seen=sw, ban=bw, penalty=P, return_logprobs=True)
    others = [i for i in range(B) if i != 1]
    np.testing.assert_array_equal(logits[others], plain[others])
    np.testing.assert_array_equal(ids[others], pids[others])
    np.testing.assert_array_equal(lp[others], plp[others])
    assert ids[1] != top and logits[1, top] == -np.inf and logits[1, 777] != plain[1, 777]
    # all-empty sets with penalty 1: the RP instantiation computes what the plain one does
    z = np.zeros_like(sw)
    l0, i0, lp0 = _call_logits(x, g, b, emb, dt, seen=z, ban=z, penalty=1.0, return_logprobs=True)
    np.testing.assert_array_equal(l0, plain)
    np.testing.assert_array_equal(i0, pids)
    np.testing.assert_array_equal(lp0, plp)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 0])
def test_sets_follow_the_history(hip, n):
    """Prompt lengths 1, 5 and 17, histories of 447, 200 and 30 ids over a small alphabet (so n-grams do repeat) and the vocabulary's
    edge ids: seen and ban equal the numpy reference after the init and after every step — a bit banned at step s is gone at s + 1
    unless it is banned again; a row past its end keeps its sets."""
    from whisper_mojo_amd import whisper_tensor as wt
    vocab = 51865
    r = np.random.default_rng(100 + n)
    alphabet = np.array([0, 31, 32, 4097, 51839, 51840, 51864])
    plen, nids = [1, 5, 17], [447, 200, 30]
    tok = np.zeros((3, 447), np.int32)
    for b in range(3):
        tok[b, :nids[b]] = r.choice(alphabet[:3 + 2 * b], nids[b])
    steps = 446
    seen, ban = wt.repeat_sets(tok, plen, nids, vocab, n, steps)
    cleared = 0
    for b in range(3):
        prev = None
        for s in range(steps + 1):
            L = min(plen[b] + s, nids[b])
            hist = tok[b, :L].tolist()
            assert set_ids(seen[s, b]) == sorted(set(hist)), (b, s)
            want = banned_ids(hist, n)
            assert set_ids(ban[s, b]) == want, (b, s, hist[-6:])
            if prev is not None:
                cleared += len(set(prev) - set(want))
            prev = want
    if n >= 2:
        assert cleared > 0  # the draw does exercise clearing
