"""Op-level tests (-m gpu) of the phrase-list constraint: the bookkeeping alone (wm_op_constraint_states: the init kernel
and the argmax launch's trie walk and mask rewrite) against the numpy restatement of tests/test_constraint_ref.py — the rows' nodes and
every mask word, bit for bit, after the init and after every step — and the processed logits of the repetition instantiation under
such a mask (wm_op_logits_processed, which the constrained pass launches with penalty 1) against float64.

Bound of the logits: tests/test_gpu_decode_ops.py's per-logit bound of the launch, as §29 / §34 use it — penalty 1 divides and
multiplies by one, so nothing is added to it; an id outside the allowed set is -inf exactly, every other id bit for bit the plain
launch's value."""
import numpy as np
import pytest

from test_constraint_ref import Table, allowed_ids, mask_words, node_of
from test_gpu_decode_ops import DT_BF16, DT_F16, DT_F32, _call_logits, _decoder_like, _logits_ref, _lowest_argmax, hip  # noqa: F401
from test_repeat_ref import banned_ids

pytestmark = pytest.mark.gpu

EOT = 17


def _table(V, free_from):
    """Edges at ids 0, 31, 32 and the last id below the free ids, on both sides of the word boundary 63 | 64; a root with 600 edges
    (more than two sweeps of the 256 threads); a fan-out-1 chain of 64 ids; phrases that are prefixes of others."""
    lim = V if free_from is None else free_from
    last = lim - 1
    ph = [(0,), (0, 31), (0, 31, 32), (0, 32), (31,), (32, last), (last,), (last, 0, 63), (last, 0, 64), (63, 64), (64, 63), (63,)]
    ph += [tuple(100 + (7 * k) % 53 for k in range(64))]                     # the chain
    ph += [(200 + k,) for k in range(600) if 200 + k not in (EOT, last)]     # the root's fan-out
    ph += [(205, 5, 6), (205, 5), (799, last, last)]
    assert all(t != EOT and t < lim for p in ph for t in p) and len(set(ph)) == len(ph)
    return Table(ph, EOT, free_from, V)


def _rows(table, r):
    """Three rows [prompt | generated]: 447 ids — free ids interleaved with the 64-id chain, then off the trie and on for hundreds of
    steps; 63 ids — a walk that ends on a phrase which goes on, with repeated 2-grams; 30 ids — the edges at the last id and at 64."""
    V, ff = table.vocab, table.free_from
    free = (lambda: int(r.integers(ff, V))) if ff < V else None
    chain = list(table.phrases[12])
    a = [3, 4, 5]
    for t in chain:
        a.append(t)
        if free:
            a += [free() for _ in range(int(r.integers(0, 3)))]
    a += [chain[0]] + [int(t) for t in r.integers(0, V, 447 - len(a) - 1)]   # the chain is a leaf: its first id again leaves the trie
    last = ff - 1
    b = [9, 8] + ([free()] if free else []) + [0] + ([free(), free()] if free else []) + [31]   # (0, 31): a phrase that goes on
    b += [0, 31, 0, 31, 0, 32, 0, 31]                                          # off the trie; 2-grams that repeat
    b += [int(t) for t in r.integers(0, 40, 63 - len(b))]
    c = [1] + [last, 0] + ([free()] if free else []) + [64] + [int(t) for t in r.integers(0, V, 25)]   # a leaf, then off the trie
    rows = [a[:447], b[:63], c[:30]]
    plen = [3, 2, 1]
    stride = max(len(x) for x in rows)
    tok = np.zeros((3, stride), np.int32)
    for i, x in enumerate(rows):
        tok[i, :len(x)] = x
    return tok, np.asarray(plen, np.int32), np.asarray([len(x) for x in rows], np.int32)


@pytest.mark.parametrize("V,free,ngram", [(1000, False, 0), (1000, True, 2), (1000, True, 1), (1000, False, 3), (51865, True, 2), (51865, False, 0),
                                          (51865, True, 1)])
def test_nodes_and_mask_words_at_every_step(hip, V, free, ngram):
    from whisper_mojo_amd import _lib, whisper_tensor as wt
    table = _table(V, V - 45 if free else None)   # (the free ids start inside a word: V - 45 is no multiple of 32)
    r = np.random.default_rng(V + 2 * free)
    tok, plen, n_ids = _rows(table, r)
    steps = int((n_ids - plen).max()) + 2          # two steps past the longest row: a finished row does nothing
    node, mask = wt.constraint_states(tok, plen, n_ids, V, table.phrases, steps, eot=EOT, free_from=table.free_from if free else None, ngram=ngram)
    trie = _lib.constraint_trie(table.phrases)
    dead = len(trie[3]) - 1
    seen_dead = seen_term = seen_both = 0
    for b in range(3):
        hist = tok[b, :n_ids[b]].tolist()
        want_node, want_mask = None, None
        for s in range(steps + 1):
            L = plen[b] + s
            if L <= n_ids[b]:       # the row stored an id at this step (or this is the init)
                gen = hist[plen[b]:L]
                want_node = node_of(gen, table, trie)
                want_mask = mask_words(gen, table, banned_ids(hist[:L], ngram) if ngram else ())
                seen_dead += want_node == dead
                ok, match = allowed_ids(gen, table)
                seen_term += match >= 0
                seen_both += match >= 0 and len([t for t in ok if t < table.free_from and t != EOT]) > 0
            assert node[s, b] == want_node, (b, s)
            bad = np.flatnonzero(mask[s, b] != want_mask)
            assert bad.size == 0, (b, s, bad[:4], mask[s, b][bad[:4]], want_mask[bad[:4]])
    assert seen_dead > 300 and seen_term >= 3 and seen_both >= 1
    # the last word is partial at both vocabularies: no bit past the vocabulary is ever set
    assert V % 32 and (mask[:, :, -1] >> np.uint32(V % 32) == 0).all()


def test_rows_are_isolated(hip):
    """every row of a B = 3 replay equals the same row replayed alone"""
    from whisper_mojo_amd import whisper_tensor as wt
    V = 1000
    table = _table(V, V - 45)
    tok, plen, n_ids = _rows(table, np.random.default_rng(5))
    steps = 70
    node, mask = wt.constraint_states(tok, plen, n_ids, V, table.phrases, steps, eot=EOT, free_from=table.free_from, ngram=2)
    assert len({tuple(node[:, b]) for b in range(3)}) == 3
    for b in range(3):
        n1, m1 = wt.constraint_states(tok[b:b + 1], plen[b:b + 1], n_ids[b:b + 1], V, table.phrases, steps, eot=EOT, free_from=table.free_from, ngram=2)
        np.testing.assert_array_equal(n1[:, 0], node[:, b])
        np.testing.assert_array_equal(m1[:, 0], mask[:, b])


def test_refusals(hip):
    from whisper_mojo_amd import _lib, whisper_tensor as wt
    tok, plen, n_ids = np.array([[1, 2, 3]], np.int32), np.array([1], np.int32), np.array([3], np.int32)
    L = _lib.lib()
    import ctypes as C
    ip, up = (lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))), (lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32)))
    node, mask = np.zeros((2, 1), np.int32), np.zeros((2, 1, 4), np.uint32)

    def call(ids, off, n, ff, eot=EOT):
        ids, off = np.asarray(ids, np.int32), np.asarray(off, np.int32)
        return L.wm_op_constraint_states(ip(node), up(mask), ip(tok), ip(plen), ip(n_ids), 1, 3, 100, eot, 0, ip(ids), ip(off), n, ff, 1)

    assert call([1, 2], [0, 2], 1, -1) == 0
    for args, word in ((([1, 2], [0, 0, 2], 2, -1), b"has 0 ids"), (([1, 100], [0, 2], 1, -1), b"vocabulary"), (([1, 2, 1, 2], [0, 2, 4], 2, -1), b"duplicate"),
                       (([1, 50], [0, 2], 1, 50), b"free id"), (([1, EOT], [0, 2], 1, -1), b"eot"), ((list(range(65)), [0, 65], 1, -1), b"has 65 ids"),
                       (([1, 2], [1, 2], 1, -1), b"offsets")):
        assert call(*args) != 0 and word in L.wm_last_error(), (args, L.wm_last_error())
    with pytest.raises(ValueError):
        wt.constraint_states(tok, plen, n_ids, 100, [], 1)


@pytest.mark.parametrize("N", [1000, 51865])
@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("dt", [DT_F32, DT_BF16, DT_F16])
def test_processed_logits_vs_float64(hip, dt, K, N):
    """The launch a constrained step runs — the repetition instantiation with penalty 1 and the constraint's words as its ban set —
    on three rows at three nodes (the root, a phrase end that goes on, the dead node): -inf exactly outside the allowed set, the
    plain launch's bits inside it, those within the launch's bound of float64, and the arg-max among the allowed ids."""
    B = 3
    table = _table(N, N - 45)
    gens = [[], [N - 40, 0, 31], [5, 5]]
    r = np.random.default_rng(31 * K + N + dt)
    x, g, b, emb = _decoder_like(r, B, K, N, dt)
    plain, _ = _call_logits(x, g, b, emb, dt)
    ban = np.stack([mask_words(gen, table) for gen in gens])
    seen = np.zeros_like(ban)
    logits, ids, lp = _call_logits(x, g, b, emb, dt, return_logprobs=True, seen=seen, ban=ban, penalty=1.0)
    ref, bound = _logits_ref(x, g, b, emb, dt)
    for bb, gen in enumerate(gens):
        ok = np.asarray(allowed_ids(gen, table)[0])
        out = np.setdiff1d(np.arange(N), ok)
        assert np.isneginf(logits[bb, out]).all()
        np.testing.assert_array_equal(logits[bb, ok], plain[bb, ok])
        assert (np.abs(logits[bb, ok] - ref[bb, ok]) <= bound[bb, ok]).all()
        assert ids[bb] in ok and ids[bb] == _lowest_argmax(logits[bb:bb + 1])[0]
        z = logits[bb, ok].astype(np.float64)
        want_lp = float(z.max() - (z.max() + np.log(np.exp(z - z.max()).sum())))   # normalised over the allowed set alone
        assert abs(float(lp[bb]) - want_lp) <= 1e-4
