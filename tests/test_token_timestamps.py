"""CPU: a numpy restatement of the token-timestamp stage (normalise, median filter, head mean, DTW, jump times) equals HF's own
times on every table of tests/golden/token_timestamps_tables.npz (made by tools/make_golden_token_timestamps.py from
WhisperGenerationMixin._extract_token_timestamps).  The GPU tests lean on this restatement for the 16-bit configurations: its
arithmetic is the kernels' (csrc/kernels_align.hip) operation for operation, so on the same weights the two agree bit for bit
(tests/test_gpu_align_chain_op.py holds the kernels to that: the matrix `normalise` returns, and the times at the DTW's edges)."""
import numpy as np
import pytest

from conftest import golden


def normalise(w):
    """w [n_sel, R, F] fp32 -> the head-averaged matrix [R, F] fp32, as align_stats / align_median compute it."""
    n_sel, R, F = w.shape
    s = np.zeros((n_sel, F), np.float64)
    for r in range(R):  # row order, float64
        s += w[:, r, :].astype(np.float64)
    mean = s / R
    v = np.zeros((n_sel, F), np.float64)
    for r in range(R):
        dv = w[:, r, :].astype(np.float64) - mean
        v += dv * dv
    mean32 = mean.astype(np.float32)
    std32 = np.sqrt(v / R).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = (w - mean32[:, None, :]) / std32[:, None, :]  # fp32
    if F > 3:  # width-7 median, reflect padding (edge not repeated); np.sort puts NaN last like torch.sort
        zp = np.concatenate([z[..., 3:0:-1], z, z[..., -2:-5:-1]], axis=-1)
        win = np.stack([zp[..., t:t + F] for t in range(7)], axis=-1)
        z = np.sort(win, axis=-1)[..., 3]
    acc = np.zeros((R, F), np.float32)
    for k in range(n_sel):  # heads in order, fp32
        acc = acc + z[k]
    return acc / np.float32(n_sel)


def dtw_jumps(m, stats=None):
    """HF _dynamic_time_warping on -m: fp32 cost, fp32(double(x) + double(c)), strict-comparison tie order; returns, per text row,
    the time index where the path enters it.  stats (a dict): stats["ties"] counts the cells whose smallest finite predecessor cost
    is held by more than one predecessor, where only the strictness of the comparisons decides."""
    ties = 0
    x = -m.astype(np.float64)
    R, F = x.shape
    cost = np.full((R + 1, F + 1), np.inf, np.float32)
    cost[0, 0] = 0
    trace = np.zeros((R + 1, F + 1), np.int8)
    for j in range(1, F + 1):
        for i in range(1, R + 1):
            c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
            if stats is not None:
                lo = min(c0, c1, c2)
                ties += bool(lo < np.inf) and int(c0 == lo) + int(c1 == lo) + int(c2 == lo) > 1
            if c0 < c1 and c0 < c2:
                c, t = c0, 0
            elif c1 < c0 and c1 < c2:
                c, t = c1, 1
            else:
                c, t = c2, 2
            cost[i, j] = np.float32(x[i - 1, j - 1] + np.float64(c))
            trace[i, j] = t
    trace[0, :] = 2
    trace[:, 0] = 1
    jt = np.zeros(R, np.int64)
    i, j = R, F
    while i > 0 or j > 0:
        if i > 0:
            jt[i - 1] = j - 1
        t = trace[i, j]
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    if stats is not None:
        stats["ties"] = int(ties)
    return jt


def restate_times(w, n_prompt, n_ids=None):
    """w [n_sel, R, F] -> float32 times of n_prompt + R + 1 ids (HF layout)."""
    n_sel, R, F = w.shape
    n = n_prompt + R + 1 if n_ids is None else n_ids
    out = np.zeros(n, np.float32)
    if R == 0:
        return out
    jt = dtw_jumps(normalise(w.astype(np.float32)))
    times = (jt.astype(np.float64) * 0.02).astype(np.float32)
    out[n_prompt:n_prompt + R] = times
    out[n_prompt + R] = times[-1]
    return out


def tables():
    g = golden("token_timestamps_tables")
    return g, [str(n) for n in g["names"]]


@pytest.mark.parametrize("name", tables()[1])
def test_restatement_equals_hf_tables(name):
    g, _ = tables()
    w = g[name + "_q"].astype(np.float32) / np.float32(65536)
    want = g[name + "_times"]
    got = restate_times(w, int(g["n_prompt"]))
    assert got.shape == want.shape
    np.testing.assert_array_equal(got, want)


def test_tables_cover_the_edges():
    g, names = tables()
    for R in (0, 1, 2, 7, 60):
        for F in (3, 8, 100, 1500):
            assert f"r{R}_f{F}" in names
    assert sum(n.startswith("tie_") for n in names) >= 3
    assert not np.any(g["r0_f100_times"])  # R = 0: HF's early return, all zeros
    w = g["r1_f100_q"].astype(np.float32) / 65536
    assert np.all(np.isnan(normalise(w)))  # R = 1: std 0, HF's 0/0 path


def test_stream_fixtures_are_self_consistent():
    """The stored probabilities of the micro streams give the stored HF times through the restatement (uncut loop, whole window)."""
    for mode in ("hf", "ref"):
        g = golden(f"token_timestamps_micro_{mode}")
        for c in range(3):
            ids = g[f"c{c}_ids"]
            p = g[f"c{c}_probs"]
            R = len(ids) - len(g["prompt"]) - 1
            np.testing.assert_array_equal(restate_times(p[:, :R], len(g["prompt"])), g[f"c{c}_times_full"])
