"""CPU: the seeded generators behind tests/test_gpu_align_chain_op.py (weight tables for the normalisation and the DTW, operands and
references for the alignment probabilities), and the proof that each of them still produces the edge it is there for: a generator
that silently stopped making NaN windows, cost ties or a covering set of shapes would otherwise leave the GPU tests green and blind."""
import functools

import numpy as np

from test_token_timestamps import dtw_jumps, normalise, restate_times

# ---- weight tables ------------------------------------------------------------------------------------------------------------


def nan_columns(F):
    """Where prob_table(..., const=True) puts its constant columns: within 3 of both edges (1 and 2 share every window around
    column 0, so some medians are NaN and some are numbers), and one in the middle."""
    if F < 4:
        return ()
    if F < 8:
        return (1, 2) if F < 6 else (1, 2, F - 2)
    return tuple(sorted({1, 2, F // 2, F - 2}))


def prob_table(seed, n_sel, R, F, const=False):
    """[n_sel, R, F] fp32 weights like probabilities: positive, peaked, rows summing to about 1, every value k / 65536 as
    tools/make_golden_token_timestamps.py stores its tables (exact in fp32, and coarse enough that equal values occur).  const: the
    columns nan_columns(F) are constant down the rows in every head, so their std is exactly 0 and their z-scores are 0/0."""
    rng = np.random.default_rng(seed)
    p = rng.random((n_sel, R, F)) ** 6 + 1e-3
    p /= p.sum(-1, keepdims=True)
    k = np.clip(np.rint(p * 65536), 1, 65535)
    w = (k / 65536).astype(np.float32)
    if const and R:
        for c in nan_columns(F):
            w[:, :, c] = w[:, :1, c]
    return w


def tie_table(seed, n_sel, R, F):
    """Two levels per column, half the rows each (R even), shuffled: every z-score is exactly +-1, so the DTW keeps comparing equal
    costs (the tie_ tables of tools/make_golden_token_timestamps.py)."""
    rng = np.random.default_rng(seed)
    w = np.zeros((n_sel, R, F), np.float32)
    for k in range(n_sel):
        for j in range(F):
            col = np.array([16384] * (R // 2) + [49152] * (R - R // 2), np.float32) / 65536
            rng.shuffle(col)
            w[k, :, j] = col
    return w


# name -> (n_sel, [(R, F, const)]): one ragged launch of wm_op_align_norm each, L = max R and T = max F.  Together: n_sel 1, 2, 6,
# 32; F 1..8, 15, 16, 17, 255, 256, 257, 1500; R 1, 2, 3, 64, 130; R_b < L and F_b < T in every launch; constant columns
NORM_LAUNCHES = {
    "sel2_l130_t257": (2, [(130, 257, False), (64, 256, False), (3, 255, False), (2, 17, False), (1, 16, False), (130, 15, False),
                           (64, 8, False), (3, 7, False), (2, 6, False), (130, 5, False), (64, 4, False), (3, 3, False), (2, 2, False),
                           (130, 1, False), (5, 100, True), (64, 257, True), (130, 8, True), (3, 5, True), (0, 9, False)]),
    "sel1_l3_t1500": (1, [(3, 1500, False), (2, 1500, True), (3, 17, False), (1, 1500, False)]),
    "sel6_l64_t17": (6, [(64, 17, False), (64, 16, True), (7, 15, False), (64, 8, True), (2, 4, False)]),
    "sel32_l5_t8": (32, [(5, 8, False), (5, 4, False), (3, 7, True), (1, 5, False), (5, 8, True)]),
    "sel2_l130_t1500": (2, [(130, 1500, True), (64, 1499, False)]),
}


@functools.lru_cache(maxsize=None)
def norm_launch(name):
    """-> (tables, packed [n_tab, n_sel, L, T] with NaN wherever no table lives, R [n_tab], F [n_tab])."""
    n_sel, specs = NORM_LAUNCHES[name]
    seed0 = 7000 + 100 * sorted(NORM_LAUNCHES).index(name)
    tabs = [prob_table(seed0 + i, n_sel, R, F, const) for i, (R, F, const) in enumerate(specs)]
    L, T = max(1, max(s[0] for s in specs)), max(s[1] for s in specs)
    packed = np.full((len(tabs), n_sel, L, T), np.nan, np.float32)
    for i, w in enumerate(tabs):
        packed[i, :, :w.shape[1], :w.shape[2]] = w
    return tabs, packed, np.asarray([s[0] for s in specs], np.int32), np.asarray([s[1] for s in specs], np.int32)


# the DTW's edges, n_sel = 2.  R 63/64/65: the second wave of align_dtw (thread i owns row i, 64 per wave); F 16/17: the 16-column
# trace word; 395 / 396 x 1500: the last trace that fits in LDS and the first in global memory; 447 = ALIGN_MAX_ROWS
DTW_SHAPES = [(63, 100), (64, 100), (65, 100), (128, 257), (447, 64), (395, 1500), (396, 1500), (447, 1500), (200, 16), (200, 17), (5, 4),
              (9, 7), (100, 30)]
DTW_TIES = [(64, 100), (130, 64)]
DTW_NAN = [(64, 100), (130, 17)]


@functools.lru_cache(maxsize=None)
def dtw_table(kind, R, F):
    if kind == "tie":
        return tie_table(9000 + R + F, 2, R, F)
    return prob_table(8000 + 7 * R + F, 2, R, F, const=kind == "nan")


def dtw_cases():
    return [("rand", R, F) for R, F in DTW_SHAPES] + [("tie", R, F) for R, F in DTW_TIES] + [("nan", R, F) for R, F in DTW_NAN]


@functools.lru_cache(maxsize=None)
def dtw_want(kind, R, F):
    """restate_times of the table with n_prompt 0 (computed once per process: the pure-Python DTW takes seconds at 447 x 1500)."""
    return restate_times(dtw_table(kind, R, F), 0)


# ---- alignment probabilities ------------------------------------------------------------------------------------------------

KINDS = ("f32", "bf16", "f16", "absorbed")
SENTINEL = np.float32(-12345.5)


def _case(kind, d, n_layers, n_sel, rows, L, T):
    return dict(kind=kind, d=d, n_layers=n_layers, n_sel=n_sel, rows=tuple(rows), B=len(rows), L=L, T=T)


PROBS_CASES = [
    _case("f32", 128, 2, 1, [1], 1, 1),
    _case("bf16", 128, 2, 1, [1], 1, 1),
    _case("absorbed", 128, 2, 1, [1], 1, 1),
    _case("f32", 384, 3, 3, [65, 0, 63], 65, 63),
    _case("f16", 384, 3, 3, [65, 0, 63], 65, 63),
    _case("absorbed", 384, 3, 3, [65, 0, 63], 65, 63),
    _case("bf16", 512, 2, 6, [64], 64, 64),
    _case("absorbed", 512, 2, 6, [64], 64, 64),
    _case("f16", 512, 2, 1, [64], 64, 64),
    _case("f16", 128, 3, 6, [130, 1, 0], 130, 65),
    _case("absorbed", 128, 3, 6, [130, 1, 0], 130, 65),
    _case("f32", 384, 2, 3, [130, 64, 0], 130, 65),
    _case("f32", 512, 3, 3, [63], 63, 257),
    _case("absorbed", 384, 2, 3, [0, 63, 2], 63, 257),
    _case("bf16", 384, 2, 1, [64, 64, 0], 64, 257),
    _case("f32", 128, 2, 3, [65], 65, 1500),
    _case("bf16", 384, 2, 3, [65], 65, 1500),
    _case("f16", 128, 3, 6, [5, 0, 3], 5, 1500),
    _case("absorbed", 512, 2, 3, [65], 65, 1500),
    _case("bf16", 128, 3, 3, [1, 130, 65], 130, 1500),
    _case("f16", 512, 3, 3, [63, 1, 64], 64, 257),
]


def case_id(c):
    return f"{c['kind']}-d{c['d']}-nl{c['n_layers']}-sel{c['n_sel']}-rows{'_'.join(map(str, c['rows']))}-L{c['L']}-T{c['T']}"


def layer_head_pairs(n_layers, H, n_sel):
    """n_sel distinct (layer, head) pairs: the last head of the last layer first; from three on also head 0 of layer 0 (another
    layer) and head 0 of the last layer (two heads of one layer); then the rest in order."""
    first = [(n_layers - 1, H - 1), (0, 0), (n_layers - 1, 0)]
    rest = [(l, h) for l in range(n_layers) for h in range(H) if (l, h) not in first]
    return np.asarray((first + rest)[:n_sel], np.int32)


def round_bf16(a):
    """fp32 -> the nearest bf16 (ties to even) as fp32, the library's upload rounding; finite inputs."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    u = (u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def round_kind(a, kind):
    if kind == "f32":
        return np.ascontiguousarray(a, np.float32)
    if kind == "f16":
        return a.astype(np.float16).astype(np.float32)
    return round_bf16(a)


LOUD_EVERY = 11  # every 11th key is 8x louder than the rest: the key an aligned row points at dominates its row


def probs_problem(c, seed=None):
    """Operands of one wm_op_align_probs call and what the kernels see of them.  Returns a dict with q [B, L, n_sel, 64], pairs, and
    either kv [n_layers, 2, B, T, d] or X [B, T, d] + Wk [n_layers, 2, d, d] (fp32, not yet rounded: the library rounds on upload), and
    K64 [B, n_sel, T, 64]: the selected heads' keys in float64 exactly as the kernels see them (cache values rounded to the cache
    type; absorbed: bf16(X)·bf16(Wk_h)ᵀ in float64, no bias).

    Every (layer, head, utterance) block of K has its own scale and its own mean vector; the V halves (of the cache, of Wk) hold
    large numbers of another scale, so any wrong offset lands on visibly different values.  Rows of q, by r % 5: 0 points at one loud
    key (score about +60, the rest O(1)); 1 points against the block's mean key (every score around -60); the others are N(0, 1)."""
    kind, d, nl, n_sel, B, L, T = c["kind"], c["d"], c["n_layers"], c["n_sel"], c["B"], c["L"], c["T"]
    H = d // 64
    rng = np.random.default_rng(sum(ord(ch) for ch in case_id(c)) if seed is None else seed)
    pairs = layer_head_pairs(nl, H, n_sel)
    out = dict(pairs=pairs)
    loud = np.where(np.arange(T) % LOUD_EVERY == 3, 8.0, 1.0)
    if kind == "absorbed":
        # K_h = X·Wk_hᵀ: the block scale sits in Wk's rows (per layer and head) and in X (per utterance), the mean key in X's mean row
        sig = 0.5 + 1.5 * rng.permutation(nl * H).reshape(nl, H) / max(1, nl * H - 1)
        Wk = np.empty((nl, 2, d, d), np.float32)
        Wk[:, 0] = rng.standard_normal((nl, d, d)) * np.repeat(sig, 64, axis=1)[:, :, None] / np.sqrt(d)
        Wk[:, 1] = rng.uniform(50, 200, (nl, d, d)) * rng.choice([-1.0, 1.0], (nl, d, d))
        X = np.empty((B, T, d), np.float32)
        for b in range(B):
            X[b] = (1 + 0.25 * b) * (4.0 * rng.standard_normal(d)[None, :] + rng.standard_normal((T, d)) * loud[:, None])
        Xr, Wr = round_bf16(X).astype(np.float64), round_bf16(Wk).astype(np.float64)
        K64 = np.stack([np.stack([Xr[b] @ Wr[l, 0, 64 * h:64 * h + 64].T for l, h in pairs]) for b in range(B)])
        out.update(X=X, Wk=Wk)
    else:
        sig = 0.5 + 1.5 * rng.permutation(nl * B * H).reshape(nl, B, H) / max(1, nl * B * H - 1)
        kv = np.empty((nl, 2, B, T, d), np.float32)
        mu = 4.0 * rng.choice([-1.0, 1.0], (nl, B, 1, d))
        kv[:, 0] = (mu + rng.standard_normal((nl, B, T, d)) * loud[None, None, :, None]) * np.repeat(sig, 64, axis=2)[:, :, None, :]
        kv[:, 1] = rng.uniform(500, 2000, (nl, B, T, d)) * rng.choice([-1.0, 1.0], (nl, B, T, d))
        kr = round_kind(kv[:, 0], kind).astype(np.float64)
        K64 = np.stack([np.stack([kr[l, b, :, 64 * h:64 * h + 64] for l, h in pairs]) for b in range(B)])
        out.update(kv=kv)
    q = rng.standard_normal((B, L, n_sel, 64)).astype(np.float32)
    for b in range(B):
        for k in range(n_sel):
            K = K64[b, k]
            m = K.mean(0)
            for r in range(L):
                if r % 5 == 0:
                    j = (7 * r + 3) % T
                    j = j - j % LOUD_EVERY + 3 if j - j % LOUD_EVERY + 3 < T else j  # the loud key of j's group, where there is one
                    dk = K[j] - m if T > 1 else K[j]  # off the mean key: the other scores stay small
                    q[b, r, k] = 480.0 * dk / (dk @ K[j])
                elif r % 5 == 1:
                    q[b, r, k] = -480.0 * m / (m @ m) + 0.1 * q[b, r, k]
    out.update(q=q, K64=K64)
    return out


def softmax_ref(q, K, dtype):
    """softmax_j(0.125·q_r·K_j) for q [R, 64], K [T, 64] in `dtype` arithmetic throughout (matmul, exp, sum)."""
    s = dtype(0.125) * (q.astype(dtype) @ K.astype(dtype).T)
    e = np.exp(s - s.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True, dtype=dtype)


def probs_refs(c, prob):
    """-> (ref64, ref32) [B, n_sel, L, T] float64, rows >= rows[b] zero.  ref64: the float64 reference on the operands as the
    kernels see them.  ref32: the same chain in numpy float32 (fp32 matmul, exp and sum; absorbed: K_h by an fp32 matmul of the
    bf16-rounded operands too) — its distance from ref64 is what fp32 arithmetic costs on this case."""
    B, n_sel, L, T = c["B"], c["n_sel"], c["L"], c["T"]
    ref64, ref32 = np.zeros((B, n_sel, L, T)), np.zeros((B, n_sel, L, T))
    for b in range(B):
        R = c["rows"][b]
        if R == 0:
            continue
        for k, (l, h) in enumerate(prob["pairs"]):
            qk = prob["q"][b, :R, k]
            ref64[b, k, :R] = softmax_ref(qk, prob["K64"][b, k], np.float64)
            if c["kind"] == "absorbed":
                K32 = round_bf16(prob["X"][b]) @ round_bf16(prob["Wk"][l, 0, 64 * h:64 * h + 64]).T
            else:
                K32 = prob["K64"][b, k].astype(np.float32)  # exact: the cache values are fp32 or narrower
            ref32[b, k, :R] = softmax_ref(qk, K32, np.float32)
    return ref64, ref32


# ---- the generators still produce their edges -----------------------------------------------------------------------------------


def _zscores(w):
    """normalise's z-scores before the median, head 0."""
    mean = w[0].astype(np.float64).mean(0)
    std = np.sqrt(((w[0].astype(np.float64) - mean) ** 2).mean(0))
    with np.errstate(invalid="ignore", divide="ignore"):
        return (w[0] - mean.astype(np.float32)) / std.astype(np.float32)


def test_norm_launches_cover_the_edges():
    specs = [(n_sel, R, F, const, name) for name, (n_sel, tabs) in NORM_LAUNCHES.items() for R, F, const in tabs]
    assert {s[0] for s in specs} == {1, 2, 6, 32}
    assert {s[2] for s in specs} >= {1, 2, 3, 4, 5, 6, 7, 8, 15, 16, 17, 255, 256, 257, 1500}
    assert {s[1] for s in specs} >= {1, 2, 3, 64, 130}
    for name in NORM_LAUNCHES:
        _, packed, R, F = norm_launch(name)
        assert (R < packed.shape[2]).any() and (F < packed.shape[3]).any(), name  # ragged in both directions
    assert sum(s[3] for s in specs) >= 6


def test_tables_look_like_probabilities_and_repeat_values():
    w = prob_table(1, 2, 64, 257)
    assert w.min() > 0 and np.abs(w.sum(-1) - 1).max() < 0.01
    np.testing.assert_array_equal(w, np.rint(w * 65536) / 65536)
    assert len(np.unique(w[0, :, 5])) < 64  # equal values within one column
    np.testing.assert_array_equal(w, prob_table(1, 2, 64, 257))  # seeded


def test_restatement_runs_on_every_generated_table():
    for name in NORM_LAUNCHES:
        for w in norm_launch(name)[0]:
            if w.shape[1]:
                assert normalise(w).shape == w.shape[1:]
    for kind, R, F in dtw_cases():
        if R * F > 50000:  # the pure-Python DTW at these sizes takes seconds each: the GPU test runs them, once
            assert normalise(dtw_table(kind, R, F)).shape == (R, F)
            continue
        t = dtw_want(kind, R, F)
        assert t.shape == (R + 1,) and np.isfinite(t).all() and (np.diff(t[:R]) >= 0).all()


def test_nan_tables_put_nan_and_numbers_into_one_median_window():
    seen_nan_median = seen_number_median = 0
    tabs = [w for name in NORM_LAUNCHES for w, s in zip(norm_launch(name)[0], NORM_LAUNCHES[name][1]) if s[2]]
    tabs += [dtw_table("nan", R, F) for R, F in DTW_NAN]
    assert len(tabs) >= 8
    for w in tabs:
        R, F = w.shape[1:]
        if R < 2:
            continue
        z = _zscores(w)
        cols = nan_columns(F)
        assert cols and min(cols) <= 3 and F - 1 - max(cols) <= 3
        for c in cols:
            assert np.isnan(z[:, c]).all()
        assert np.isfinite(np.delete(z, cols, axis=1)).any()  # (a coarse column may be constant by chance as well)
        zp = np.concatenate([z[:, 3:0:-1], z, z[:, -2:-5:-1]], axis=1)
        mixed = 0
        for j in range(F):
            win = zp[0, j:j + 7]
            n_nan = int(np.isnan(win).sum())
            if 0 < n_nan < 7:
                mixed += 1
                seen_nan_median += n_nan >= 4
                seen_number_median += n_nan < 4
        assert mixed > 0
        # a window on the reflected side of an edge: column 0's window holds column 1 twice
        assert np.isnan(zp[0, 0:7]).any() and np.isfinite(zp[0, 0:7]).any()
        m = normalise(w)
        assert np.isnan(m).any() and np.isfinite(m).any()
    assert seen_nan_median and seen_number_median


def test_tie_tables_tie():
    for R, F in DTW_TIES:
        w = dtw_table("tie", R, F)
        m = normalise(w)
        assert set(np.unique(m)) <= {-1.0, 0.0, 1.0}
        stats = {}
        dtw_jumps(m, stats)
        assert stats["ties"] > 0
        print(f"tie table {R} x {F}: {stats['ties']} tied cells")


def test_probs_cases_cover_the_issue():
    cs = PROBS_CASES
    assert 20 <= len(cs) <= 30 and len({case_id(c) for c in cs}) == len(cs)

    def kinds_with(pred):
        return {c["kind"] for c in cs if pred(c)}
    for d in (128, 384, 512):
        assert len(kinds_with(lambda c: c["d"] == d)) >= 2
    for v in (2, 3):
        assert len(kinds_with(lambda c: c["n_layers"] == v)) >= 2
    for v in (1, 3, 6):
        assert len(kinds_with(lambda c: c["n_sel"] == v)) >= 2
    for v in (1, 3):
        assert len(kinds_with(lambda c: c["B"] == v)) >= 2
    assert len(kinds_with(lambda c: c["B"] == 3 and 0 in c["rows"] and len(set(c["rows"])) == 3)) >= 2
    for T in (1, 63, 64, 65, 257):
        assert len(kinds_with(lambda c: c["T"] == T)) >= 2
    assert kinds_with(lambda c: c["T"] == 1500) == set(KINDS)
    for v in (1, 63, 64, 65, 130):
        assert len(kinds_with(lambda c: c["L"] == v)) >= 2
        assert len(kinds_with(lambda c: v in c["rows"])) >= 2
    assert len(kinds_with(lambda c: any(0 < r and -(-r // 64) < -(-c["L"] // 64) for r in c["rows"]))) >= 2  # a 64-row tile that exits early
    for c in cs:
        if c["T"] <= 65:  # (the wide ones cost a second each; their operands are made by the same code)
            prob = probs_problem(c)
            assert np.isfinite(prob["q"]).all() and np.isfinite(prob["K64"]).all() and np.isfinite(probs_refs(c, prob)[1]).all()
        p = layer_head_pairs(c["n_layers"], c["d"] // 64, c["n_sel"])
        assert len({tuple(x) for x in p}) == c["n_sel"] and tuple(p[0]) == (c["n_layers"] - 1, c["d"] // 64 - 1)
        if c["n_sel"] >= 3:
            assert len(set(p[:, 0])) > 1 and (0, 0) in {tuple(x) for x in p} and np.bincount(p[:, 0]).max() >= 2


def test_probs_operands_stress_the_softmax():
    """The aligned rows reach about +60 with the rest far below, the negative rows sit around -60, the 16-bit roundings are finite,
    and the V halves are of another scale than K."""
    for c in (PROBS_CASES[4], PROBS_CASES[9], PROBS_CASES[10]):
        prob = probs_problem(c)
        np.testing.assert_array_equal(prob["q"], probs_problem(c)["q"])  # seeded
        b = int(np.argmax(c["rows"]))
        s = 0.125 * prob["q"][b, :, 0].astype(np.float64) @ prob["K64"][b, 0].T
        assert abs(s[0].max() - 60) < 1 and np.sort(s[0])[-2] < 30
        assert -90 < s[1].mean() < -30 and s[1].max() < 0
        assert np.abs(s[2]).max() < 60
        if "kv" in prob:
            assert np.isfinite(prob["kv"].astype(np.float16)).all()
            assert np.abs(prob["kv"][:, 1]).min() >= 500 > 20 * np.abs(prob["kv"][:, 0]).mean()
        else:
            assert np.abs(prob["Wk"][:, 1]).min() >= 50 > 100 * np.abs(prob["Wk"][:, 0]).mean()
        ref64, ref32 = probs_refs(c, prob)
        R = c["rows"][b]
        np.testing.assert_allclose(ref64[b, :, :R].sum(-1), 1, atol=1e-12)
        assert np.abs(ref32 - ref64).max() < 1e-3
