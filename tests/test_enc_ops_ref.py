"""CPU side of the encoder attention / LayerNorm op tests (the GPU side is tests/test_gpu_enc_attn_ln_op.py).

Holds the seeded case generators, the float64 references, the per-element error bounds and numpy float32 restatements of the
arithmetic of flash_attn_enc_v2_kernel, flash_attn_enc_kernel and layernorm_rows_kernel.  The tests here prove without a GPU that
the restatement alone stays inside every bound on every case and that every generator still hits the edge it is there for — so a
GPU test that fails, fails because of the kernel.

Attention bound, per output element (A = softmax·|V|, u_T = 2^-9 bf16, 2^-12 f16, 0 fp32; the factor 2 in front makes u_T the
format's half-ulp 2^-8 / 2^-11):
    the kernel sums l from unrounded p (fp32 error only); the numerator uses p rounded to T: at most u_T·A; the output store adds
    u_T·|ref|; MFMA accumulation over n_ctx keys, v_exp_f32 and the division add a term of order n_ctx·2^-24·A:
        bar = 2·(u_T·(A + |ref|) + n_ctx·2^-24·A)
    f16 only: "relative error at most u_T" fails for p below f16's smallest normal number 2^-14, where the spacing is 2^-24 whatever p
    is (the restatement left the bar above by 1.8x on the spike of 2^20 in the last tile: 62 flat keys at p = 2^-20 next to it).  The
    reference m is a past maximum of the row, so the kernel's p is at least p against the row's final maximum and l >= 1 after every
    refresh: such a key adds at most 2^-25·|v_j|, and only where its p against the row maximum is below 2^-14:
        bar_f16 = bar + 2^-25·Σ_{j: p_j / p_max < 2^-14} |v_j|
LayerNorm bound, per element, from the kernel's summation order (4·V4 sequential adds per lane, 5 butterfly levels, one-pass
variance), u = 2^-24, c = 4·V4 + 7:
    Δvar <= c·u·(E[x²] + mean²);  rel(inv_std) <= Δvar / (2 (var + eps)) + 4 ulp;  Δmean <= c·u·E|x|
    |Δy| <= |g|·inv_std·(Δmean + |x - mean|·(rel + 3u)) + u·|y|          (out_t: + half an ulp of T at |y| + |Δy|)
"""
import functools
import zlib

import numpy as np
import pytest

U = {"f32": 0.0, "bf16": 2.0 ** -9, "f16": 2.0 ** -12}
HALF_ULP = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}
DTYPE = {"f32": 0, "bf16": 1, "f16": 2}
DTYPES = ("bf16", "f16", "f32")
SENTINEL = np.float32(-77.5)  # exact in bf16 and f16
LOG2E = 1.4426950408889634
SL = np.float32(np.float32(0.125) * np.float32(LOG2E))  # the launcher's scale·log2e


def bf16_round(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def rnd(a, dt):
    """a rounded to the operand type (round to nearest even, as the upload and the kernels' stores do), as float32."""
    a = np.ascontiguousarray(a, np.float32)
    if dt == "bf16":
        return bf16_round(a)
    if dt == "f16":
        with np.errstate(over="ignore"):
            return a.astype(np.float16).astype(np.float32)
    return a


def _rng(tag):
    return np.random.default_rng(zlib.crc32(tag.encode()))


# ---------------------------------------------------------------------------------------------------------------------------------
# attention cases

def A(pat, n, H, B, **kw):
    return dict(pat=pat, n=n, H=H, B=B, **kw)


def case_id(c):
    return "-".join(str(c[k]) for k in ("pat", "n", "H", "B")) + "".join(f"-{k}{v}" for k, v in sorted(c.items()) if k not in ("pat", "n", "H", "B"))


# A covering subset of n_ctx {1, 15..17, 63..65, 127..129, 191, 257} x H {1, 2, 6, 8, 12} x B {1..4}.  The XCD remap is on when
# B·H % 8 == 0: npair/8 = 1 (8-1, 2-4), 2 (8-2), 3 (6-4, 12-2); off for 1-1, 2-3, 6-3, 12-1, 6-1, 2-1.
ATTN_CASES = [
    A("random", 1, 1, 1), A("random", 15, 2, 3), A("random", 16, 6, 4), A("random", 17, 12, 2), A("random", 63, 8, 2),
    A("random", 64, 6, 3), A("random", 65, 8, 1), A("random", 127, 2, 4), A("random", 128, 12, 1), A("random", 129, 6, 4),
    A("random", 191, 8, 2), A("random", 257, 12, 2), A("random", 1500, 12, 2),
    A("growing", 191, 6, 4), A("growing", 257, 2, 1), A("outlier", 129, 8, 2), A("outlier", 257, 6, 1),
    A("stair_up", 257, 8, 2, step=9), A("stair_up", 257, 12, 2, step=10), A("stair_up", 191, 6, 4, step=11), A("stair_up", 129, 2, 3, step=40),
    A("stair_down", 257, 12, 2, step=9), A("stair_down", 257, 8, 2, step=10), A("stair_down", 191, 6, 3, step=11), A("stair_down", 129, 1, 1, step=40),
    A("spike_last", 63, 2, 4, lev=0), A("spike_last", 65, 8, 2, lev=0), A("spike_last", 127, 6, 4, lev=20), A("spike_last", 129, 12, 2, lev=0),
    A("spike_last", 191, 1, 1, lev=0), A("spike_last", 257, 8, 2, lev=20), A("spike_first", 65, 1, 2), A("spike_first", 257, 12, 2),
]
STAIR_CASES = [c for c in ATTN_CASES if c["pat"].startswith("stair")]
STAIR_KEYS = (0, 21, 42, 63)  # one key of every lane group g = (key % 16) / 4 of a 64-key tile: a lane's partial sum holds one
LOW = 30.0                    # other keys lie 30 (log2 units) under the lowest stair


def _raw(level_log2):
    """the dimension-0 key value whose score against q0 = 1 is level_log2 in the kernel's log2 units; bf16-exact, so every T holds it"""
    return bf16_round(np.asarray(level_log2, np.float64) / (0.125 * LOG2E))


@functools.lru_cache(maxsize=None)
def _attn_case(cid):
    c = next(x for x in ATTN_CASES if case_id(x) == cid)
    pat, n, H, B = c["pat"], c["n"], c["H"], c["B"]
    r = _rng(cid)
    d = 64 * H
    q, k, v = (r.standard_normal((B, n, d)).astype(np.float32) for _ in range(3))
    if pat == "growing":  # tests/test_gpu_parity.py's: key j = u·0.4 j + noise, scores keep outgrowing (or falling under) every earlier maximum
        for b in range(B):
            u = r.standard_normal(d).astype(np.float32)
            u /= np.linalg.norm(u.reshape(H, 64), axis=1).repeat(64)
            k[b] = (u[None, :] * (0.4 * np.arange(n, dtype=np.float32))[:, None]).astype(np.float32) + 0.1 * k[b]
    elif pat == "outlier":  # one key in a middle tile beats everything by ~2^100 for one row block and is hugely negative for another
        for b in range(B):
            k[b, n // 2 + 3] = 12.0 * np.sign(q[b, n // 3])
    elif pat != "random":
        # dimension 0 of every head carries a level per key: q0 = 1 + j/128 (one j per 16-row block, the rows of one wave),
        # so row i sees key j at level[j]·q0 (+ the other 63 dimensions' small noise where the key has any)
        q4, k4 = q.reshape(B, n, H, 64), k.reshape(B, n, H, 64)
        q4[..., 1:] *= 0.5
        blocks = (n + 15) // 16
        jit = r.integers(-3, 4, (B, blocks, H)).astype(np.float32) / 128
        q4[..., 0] = 1.0 + np.repeat(jit, 16, axis=1)[:, :n]
        nt = (n + 63) // 64
        if pat in ("stair_up", "stair_down"):
            lev_t = c["step"] * (np.arange(nt) - (nt - 1) / 2.0) * (1 if pat == "stair_up" else -1)
            k4[..., 0] = _raw(lev_t.min() - LOW)
            for t in range(nt):
                for o in STAIR_KEYS:
                    if t * 64 + o < n:
                        k4[:, t * 64 + o, :, 1:] = 0
                        k4[:, t * 64 + o, :, 0] = _raw(lev_t[t])
        else:  # flat scores and one spike
            k4[..., 1:] *= 0.05
            k4[..., 0] = 0
            if pat == "spike_last":  # lev 0: the spike holds half of the row's mass — a key counted twice or not at all shows
                k4[:, n - 1, :, 0] = _raw(c["lev"] if c["lev"] else np.log2(n - 1))
            else:
                k4[:, 0, :, 0] = _raw(12.0)
    for a in (q, k, v):
        a.setflags(write=False)
    return q, k, v


def attn_case(c):
    """q, k, v [B, n, 64·H] float32 (read-only; not yet rounded to an operand type).  Utterances carry different data."""
    return _attn_case(case_id(c))


@functools.lru_cache(maxsize=None)
def _attn_ref(cid, dt):
    c = next(x for x in ATTN_CASES if case_id(x) == cid)
    q, k, v = attn_case(c)
    return attn_ref64(q, k, v, c["H"], dt)


def attn_ref64(q, k, v, H, dt):
    """layers.mojo:273-342 in float64 on the operands rounded to dt: ref = softmax(q_h·k_hᵀ·0.125)·v_h and A = softmax·|v_h|."""
    q, k, v = (rnd(a, dt).astype(np.float64) for a in (q, k, v))
    B, n, d = q.shape
    q, k, v = (a.reshape(B, n, H, 64).transpose(0, 2, 1, 3) for a in (q, k, v))
    s = (q @ k.transpose(0, 1, 3, 2)) * 0.125
    s -= s.max(-1, keepdims=True)
    p = np.exp(s)
    sub = (p < 2.0 ** -14) @ np.abs(v)  # Σ|v_j| over the keys whose p against the row maximum is below f16's smallest normal number
    p /= p.sum(-1, keepdims=True)
    ref, Ab = p @ v, p @ np.abs(v)
    back = lambda a: np.ascontiguousarray(a.transpose(0, 2, 1, 3)).reshape(B, n, d)
    return back(ref), back(Ab), back(sub)


def attn_ref(c, dt):
    return _attn_ref(case_id(c), dt)


def attn_bar(ref, Ab, sub, n, dt):
    bar = 2.0 * (U[dt] * (Ab + np.abs(ref)) + n * 2.0 ** -24 * Ab)
    return bar + 2.0 ** -25 * sub if dt == "f16" else bar


def attn_ratio(got, c, dt):
    """largest error / bar over the output of case c"""
    ref, Ab, sub = attn_ref(c, dt)
    return float((np.abs(got.astype(np.float64) - ref) / attn_bar(ref, Ab, sub, c["n"], dt)).max())


def _f32(a):
    return np.asarray(a, np.float32)


def restate_v2(q, k, v, H, dt, count=None):
    """flash_attn_enc_v2_kernel<T, 8, 1> step by step in numpy float32, all (utterance, head) pairs at once: 64-key tiles, the last one
    masked with -1e30; p = exp2(fma(s, scale·log2e, -m)) against the reference m as it stands; the lane (row, g) sums its 16 scores
    (keys 16 kb + 4 g + r) as ps4[r] = Σ_kb, (ps4[0] + ps4[1]) + (ps4[2] + ps4[3]); a wave (16 rows x 4 groups) refreshes m to the running
    maximum when any of its lanes' sums fails <= 1024; l sums unrounded p per lane; the numerator takes p rounded to T.
    count: dict that receives 'refresh' / 'skip' = (wave, tile) pairs after the first tile that took / skipped the refresh."""
    q, k, v = (rnd(a, dt) for a in (q, k, v))
    B, n, d = q.shape
    npad = (n + 15) // 16 * 16
    q, k, v = (a.reshape(B, n, H, 64).transpose(0, 2, 1, 3) for a in (q, k, v))  # [B, H, n, 64]
    qp = np.concatenate([q, np.repeat(q[:, :, -1:], npad - n, axis=2)], axis=2)   # rows past n_ctx load row n_ctx - 1
    m = np.full((B, H, npad), -1e30, np.float32)
    l = np.zeros((B, H, npad, 4), np.float32)
    o = np.zeros((B, H, npad, 64), np.float32)
    nt = (n + 63) // 64
    if count is not None:
        count.update(refresh=0, skip=0)

    def probs(s, mm):
        with np.errstate(over="ignore"):
            a = _f32(s.astype(np.float64) * np.float64(SL) - mm.astype(np.float64)[..., None])  # one rounding: the fma
            p = np.exp2(a)
        p4 = p.reshape(p.shape[:-1] + (4, 4, 4))  # [.., kb, g, r]
        ps = p4[..., 0, :, :]
        for kb in range(1, 4):
            ps = ps + p4[..., kb, :, :]
        return p, (ps[..., 0] + ps[..., 1]) + (ps[..., 2] + ps[..., 3])  # [.., 64], [.., g]

    for t in range(nt):
        idx = np.minimum(np.arange(t * 64, t * 64 + 64), n - 1)  # staging clamps to the last valid key row
        kt, vt = k[:, :, idx], v[:, :, idx]
        s = _f32(qp @ kt.transpose(0, 1, 3, 2))  # float32 operands, float32 accumulation
        if t == nt - 1:
            s = np.where(np.arange(t * 64, t * 64 + 64) >= n, np.float32(-1e30), s)
        p, psum = probs(s, m)
        with np.errstate(invalid="ignore"):
            lane_bad = ~(psum <= 1024.0)  # [B, H, npad, 4]
        wave_bad = lane_bad.reshape(B, H, npad // 16, 64).any(-1)
        if count is not None and t > 0:
            count["refresh"] += int(wave_bad.sum())
            count["skip"] += int((~wave_bad).sum())
        rb = np.repeat(wave_bad, 16, axis=2)  # per row
        m_new = np.maximum(m, s.max(-1) * SL)
        alpha = np.exp2(m - m_new)
        p2, psum2 = probs(s, m_new)
        p = np.where(rb[..., None], p2, p)
        psum = np.where(rb[..., None], psum2, psum)
        l = np.where(rb[..., None], l * alpha[..., None], l)
        o = np.where(rb[..., None], o * alpha[..., None], o)
        m = np.where(rb, m_new, m)
        l = l + psum
        o = o + _f32(rnd(p, dt) @ vt)
    lt = (l[..., 0] + l[..., 1]) + (l[..., 2] + l[..., 3])
    out = rnd(o * (np.float32(1.0) / lt)[..., None], dt)[:, :, :n]
    return np.ascontiguousarray(out.transpose(0, 2, 1, 3)).reshape(B, n, d)


def restate_v1(q, k, v, H):
    """flash_attn_enc_kernel<float, false> in numpy float32: exact running maximum on every 64-key tile, p = exp(s·scale - m), the lane's
    16 p summed in order, l = l·alpha + psum per lane, no rounding of p."""
    q, k, v = (_f32(a) for a in (q, k, v))
    B, n, d = q.shape
    q, k, v = (a.reshape(B, n, H, 64).transpose(0, 2, 1, 3) for a in (q, k, v))
    m = np.full((B, H, n), -1e30, np.float32)
    l = np.zeros((B, H, n, 4), np.float32)
    o = np.zeros((B, H, n, 64), np.float32)
    for t in range((n + 63) // 64):
        idx = np.minimum(np.arange(t * 64, t * 64 + 64), n - 1)
        s = _f32(q @ k[:, :, idx].transpose(0, 1, 3, 2)) * np.float32(0.125)
        s = np.where(np.arange(t * 64, t * 64 + 64) >= n, np.float32(-1e30), s)
        m_new = np.maximum(m, s.max(-1))
        alpha = np.exp(m - m_new)
        p = np.exp(s - m_new[..., None])
        p4 = p.reshape(p.shape[:-1] + (4, 4, 4))
        ps = np.zeros(p.shape[:-1] + (4,), np.float32)
        for kb in range(4):
            for r in range(4):
                ps = ps + p4[..., kb, :, r]
        l = l * alpha[..., None] + ps
        o = o * alpha[..., None] + _f32(p @ v[:, :, idx])
        m = m_new
    lt = (l[..., 0] + l[..., 1]) + (l[..., 2] + l[..., 3])  # shfl_xor 16 then 32
    out = o * (np.float32(1.0) / lt)[..., None]
    return np.ascontiguousarray(out.transpose(0, 2, 1, 3)).reshape(B, n, d)


def restate(c, dt, count=None):
    q, k, v = attn_case(c)
    return restate_v1(q, k, v, c["H"]) if dt == "f32" else restate_v2(q, k, v, c["H"], dt, count)


# the exact selector: keys are sign vectors ·2, q_i = 4·k_perm(i) — the score of key perm(i) is 128 (nat), every other key's at most
# 2·(64 - 2·hamming)... far below; values are multiples of 1/8 with 1 <= |v| <= 4, exact in every T and never 0
SELECT_CASES = [dict(n=129, H=12, B=2), dict(n=257, H=8, B=2)]


@functools.lru_cache(maxsize=None)
def _select_case(n, H, B):
    r = _rng(f"select-{n}-{H}-{B}")
    k = (2.0 * r.choice([-1.0, 1.0], (B, n, H, 64))).astype(np.float32)
    perm = np.stack([[r.permutation(n) for _ in range(H)] for _ in range(B)])  # [B, H, n]: row i of (b, h) selects key perm[b, h, i]
    q = np.empty_like(k)
    for b in range(B):
        for h in range(H):
            q[b, :, h] = 4.0 * k[b, perm[b, h], h]
    v = (r.integers(8, 33, (B, n, H, 64)) * r.choice([-1.0, 1.0], (B, n, H, 64)) / 8.0).astype(np.float32)
    want = np.empty_like(v)
    for b in range(B):
        for h in range(H):
            want[b, :, h] = v[b, perm[b, h], h]
    return tuple(a.reshape(B, n, 64 * H) for a in (q, k, v, want)) + (perm,)


def select_case(c):
    return _select_case(c["n"], c["H"], c["B"])


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm cases

LN_COLS = tuple(range(128, 1025, 128))
LN_ROWS = (1, 2, 7, 8, 9, 17)
LN_KINDS = ("standard", "shift1", "shift30", "shift1000", "outlier")
CONST_MEANS = (1.0, 13.0, 100.0)
EPS = 1e-5


def ln_case(kind, rows, cols):
    """x [rows, cols], gamma and beta of mixed sign, float32"""
    r = _rng(f"ln-{kind}-{rows}-{cols}")
    x = r.standard_normal((rows, cols)).astype(np.float32)
    if kind.startswith("shift"):  # mean / std = 1, 30, 1000 (standardised rows + a shift just above): the one-pass variance cancels
        z = x.astype(np.float64)
        z = (z - z.mean(1, keepdims=True)) / z.std(1, keepdims=True)
        x = (z + 1.001 * float(kind[5:])).astype(np.float32)
    elif kind == "outlier":
        x[rows // 2, (7 * cols) // 11] = 1e4
    g = (r.standard_normal(cols) * 1.5).astype(np.float32)
    b = r.standard_normal(cols).astype(np.float32)
    return x, g, b


def ln_const_case(cols):
    """rows whose float64 variance is 0 (constant: the means of CONST_MEANS, then the same + a fraction float32 cannot sum exactly) or as
    good as 0 (near-constant: one element one ulp up)"""
    r = _rng(f"ln-const-{cols}")
    vals = [np.float32(m) for m in CONST_MEANS] + [np.float32(m + 0.7) for m in CONST_MEANS]
    x = np.stack([np.full(cols, v, np.float32) for v in vals] * 2)
    for i in range(len(vals), 2 * len(vals)):
        x[i, (5 * cols) // 7] = np.nextafter(x[i, 0], np.float32(np.inf))
    g = (r.standard_normal(cols) * 1.5).astype(np.float32)
    b = r.standard_normal(cols).astype(np.float32)
    return x, g, b


def ln_ref_bound(x, g, b, eps=EPS, dt=None):
    """float64 LayerNorm and the per-element bound of the module docstring (dt: the bound of the out_t store)"""
    x, g, b = (np.asarray(a, np.float64) for a in (x, g, b))
    cols = x.shape[1]
    u, cn = 2.0 ** -24, 4 * (cols // 128) + 7
    mean = x.mean(1, keepdims=True)
    ex2 = (x * x).mean(1, keepdims=True)
    dev = x - mean
    var = (dev * dev).mean(1, keepdims=True)
    istd = 1.0 / np.sqrt(var + eps)
    y = dev * istd * g + b
    dvar = cn * u * (ex2 + mean * mean)
    rel = dvar / (2.0 * (var + eps)) + 4 * 2.0 ** -23
    dmean = cn * u * np.abs(x).mean(1, keepdims=True)
    bound = np.abs(g) * istd * (dmean + np.abs(dev) * (rel + 3 * u)) + u * np.abs(y)
    if dt is not None:
        bound = bound + HALF_ULP[dt] * (np.abs(y) + bound)
    return y, bound


def ln_restate(x, g, b, eps=EPS, clamp=True):
    """layernorm_rows_kernel<T, V4> in numpy float32: lane l of the row's 32 holds x[4 (l + 32 i) + j]; Σx and Σx² over i then j in order,
    a butterfly over offsets 16..1, mean = s / cols, var = q / cols - mean², (clamp: max(var, 0),) 1 / sqrt(var + eps),
    (x - mean)·inv_std·g + b.  Returns y and the variance before the clamp."""
    x, g, b = (_f32(a) for a in (x, g, b))
    rows, cols = x.shape
    xl = x.reshape(rows, cols // 128, 32, 4)
    s = np.zeros((rows, 32), np.float32)
    q = np.zeros((rows, 32), np.float32)
    for i in range(cols // 128):
        for j in range(4):
            s = s + xl[:, i, :, j]
            q = q + xl[:, i, :, j] * xl[:, i, :, j]
    lanes = np.arange(32)
    for o in (16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ o]
        q = q + q[:, lanes ^ o]
    mean = s[:, :1] / np.float32(cols)
    var = q[:, :1] / np.float32(cols) - mean * mean
    v = np.maximum(var, np.float32(0)) if clamp else var
    with np.errstate(invalid="ignore", divide="ignore"):
        inv = np.float32(1.0) / np.sqrt(v + np.float32(eps))
    return (x - mean) * inv * g + b, var


def ln_ratio(got, x, g, b, dt=None):
    y, bound = ln_ref_bound(x, g, b, EPS, dt)
    return float((np.abs(got.astype(np.float64) - y) / bound).max())


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU tests

@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("c", ATTN_CASES, ids=case_id)
def test_attention_restatement_meets_the_bar(c, dt):
    """The kernels' arithmetic restated in float32 stays inside the derived bar on every case the GPU test runs."""
    out = restate(c, dt)
    assert np.isfinite(out).all()
    ratio = attn_ratio(out, c, dt)
    print(f"restatement {case_id(c)} {dt}: error / bar = {ratio:.3f}")
    assert ratio <= 1.0, ratio


def test_cases_cover_what_they_are_there_for():
    ns = {c["n"] for c in ATTN_CASES}
    assert {1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 257, 1500} <= ns
    assert {c["H"] for c in ATTN_CASES} == {1, 2, 6, 8, 12} and {c["B"] for c in ATTN_CASES} == {1, 2, 3, 4}
    remap = {c["B"] * c["H"] // 8 for c in ATTN_CASES if c["B"] * c["H"] % 8 == 0}
    assert {1, 2, 3} <= remap and any(c["B"] * c["H"] % 8 for c in ATTN_CASES)
    assert any((c["n"], c["H"], c["B"]) == (1500, 12, 2) for c in ATTN_CASES)
    assert {c["step"] for c in STAIR_CASES if c["pat"] == "stair_up"} == {9, 10, 11, 40} == {c["step"] for c in STAIR_CASES if c["pat"] == "stair_down"}
    assert {c["n"] % 64 for c in ATTN_CASES if c["pat"] == "spike_last"} == {1, 63}
    for c in ATTN_CASES:  # utterances carry different data
        q, k, v = attn_case(c)
        assert all(not np.array_equal(v[0], v[b]) for b in range(1, c["B"]))


@pytest.mark.parametrize("dt", ("bf16", "f16"))
def test_staircases_straddle_the_refresh_threshold(dt):
    """After the first tile the restatement takes the refresh on some (wave, tile) pairs and skips it on others: over all staircases, in
    the rising ones alone, and inside the one whose step sits on the 2^10 threshold."""
    tot = {}
    for c in STAIR_CASES:
        cnt = {}
        restate(c, dt, cnt)
        tot[case_id(c)] = cnt
        print(case_id(c), dt, cnt)
    up = [v for k_, v in tot.items() if k_.startswith("stair_up")]
    assert sum(v["refresh"] for v in up) > 0 and sum(v["skip"] for v in up) > 0
    on = next(v for k_, v in tot.items() if k_.startswith("stair_up") and k_.endswith("step10"))
    assert on["refresh"] > 0 and on["skip"] > 0
    over = next(v for k_, v in tot.items() if k_.startswith("stair_up") and k_.endswith("step40"))
    assert over["skip"] == 0 and over["refresh"] > 0
    for k_, v in tot.items():  # falling scores never outgrow the reference
        if k_.startswith("stair_down"):
            assert v["refresh"] == 0 and v["skip"] > 0


@pytest.mark.parametrize("c", SELECT_CASES, ids=lambda c: f"{c['n']}-{c['H']}-{c['B']}")
def test_selector_puts_all_mass_on_one_key(c):
    """float64 off-target probability mass below 2^-30 in every row, values exact in every operand type and never 0, permutations that
    cross tiles and differ between heads and utterances."""
    q, k, v, want, perm = select_case(c)
    n, H, B = c["n"], c["H"], c["B"]
    for a in (q, k, v):
        assert np.array_equal(bf16_round(a), a) and np.array_equal(rnd(a, "f16"), a)
    assert np.abs(v).min() >= 1.0
    s = np.einsum("bihd,bjhd->bhij", q.reshape(B, n, H, 64).astype(np.float64), k.reshape(B, n, H, 64).astype(np.float64)) * 0.125
    s -= s.max(-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(-1, keepdims=True)
    on = np.take_along_axis(p, perm[..., None], -1)[..., 0]
    assert (1.0 - on).max() < 2.0 ** -30 and (p.sum(-1) - on).max() < 2.0 ** -30
    assert (perm // 64 != np.arange(n) // 64).mean() > 0.4                      # crosses tiles
    assert not np.array_equal(perm[0, 0], perm[0, 1]) and not np.array_equal(perm[0, 0], perm[1, 0])
    for dt in DTYPES:
        got = restate_v1(q, k, v, H) if dt == "f32" else restate_v2(q, k, v, H, dt)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), dt


@pytest.mark.parametrize("cols", LN_COLS)
@pytest.mark.parametrize("kind", LN_KINDS)
def test_layer_norm_restatement_meets_the_bound(kind, cols):
    worst = 0.0
    for rows in LN_ROWS:
        x, g, b = ln_case(kind, rows, cols)
        y, var = ln_restate(x, g, b)
        assert np.isfinite(y).all()
        worst = max(worst, ln_ratio(y, x, g, b))
        for dt in ("bf16", "f16"):
            worst = max(worst, ln_ratio(rnd(y, dt), x, g, b, dt))
    print(f"layer_norm restatement {kind} cols {cols}: error / bound = {worst:.3f}")
    assert worst <= 1.0


def test_layer_norm_shifted_rows_reach_their_ratio():
    for kind, want in (("shift1", 1.0), ("shift30", 30.0), ("shift1000", 1000.0)):
        for cols in LN_COLS:
            for rows in LN_ROWS:
                x = ln_case(kind, rows, cols)[0].astype(np.float64)
                ratio = np.abs(x.mean(1)) / x.std(1)
                assert (ratio >= want).all() and (ratio <= 1.01 * want).all(), (kind, cols, ratio)


@pytest.mark.parametrize("cols", LN_COLS)
def test_layer_norm_constant_rows(cols):
    """Rows of float64 variance 0: the one-pass variance in float32 may come out below -eps (the square root of a negative number);
    with the variance clamped at 0 the result is finite and inside the bound, and the clamp changes nothing where var >= 0."""
    x, g, b = ln_const_case(cols)
    x64 = x.astype(np.float64)
    assert (x64.var(1)[:6] == 0).all() and (x64.var(1)[6:] < 1e-10).all()
    y, var = ln_restate(x, g, b)
    assert np.isfinite(y).all()
    ratio = ln_ratio(y, x, g, b)
    print(f"constant rows cols {cols}: min var {var.min():.3e}, error / bound = {ratio:.3f}")
    assert ratio <= 1.0
    y0, _ = ln_restate(x, g, b, clamp=False)
    keep = (var >= 0)[:, 0]
    assert np.array_equal(y0[keep].view(np.uint32), y[keep].view(np.uint32))
