"""CPU-only: the float64 absorbed cross-attention reference of tests/test_gpu_decode_ops.py equals the direct (cached K/V) form
of the same attention, so the GPU test's reference is the attention it claims to be."""
import numpy as np

from test_gpu_decode_layer import gelu64, linear_ref, ln_depth, prefill_counts, qkv_scatter, store16
from test_gpu_decode_ops import DT_BF16, DT_F16, DT_F32, _decoder_like, _round, _ulp_tw, xattn_ref, xattn_ref_direct
from test_gpu_parity import _attention_cached_ref as attention_cached_ref


def test_absorbed_reference_equals_direct_form():
    r = np.random.default_rng(5)
    for H, n_keys, rows, q_B in ((1, 7, 2, 0), (3, 40, 4, 2), (2, 1, 1, 0)):
        d = 64 * H
        q = r.standard_normal((rows, d)).astype(np.float32)
        Wk = (r.standard_normal((d, d)) * 2 / np.sqrt(d)).astype(np.float32)
        Wv = (r.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32)
        bv = r.standard_normal(d).astype(np.float32)
        X = r.standard_normal((q_B if q_B else rows, n_keys, d)).astype(np.float32)
        a = xattn_ref(q, Wk, Wv, bv, X, H, q_B)
        b = xattn_ref_direct(q, Wk, Wv, bv, X, H, q_B)
        assert np.abs(a - b).max() < 1e-12 * max(1.0, np.abs(b).max())


# ---- the references and bounds of tests/test_gpu_decode_layer.py ----------------------------------------------------------------



def test_linear_reference_equals_oracle_compositions():
    """linear_ref (fp32 operands: no rounding of a or W) against the oracle's layer_norm / matmul / gelu compositions.  The oracle
    computes in fp32, so agreement is to fp32 accuracy: 2e-5 of Σ|a||w| + |bias| per element (K <= 384 fp32 products and adds)."""
    from oracle import oracle
    r = np.random.default_rng(11)
    for K, N, B in ((128, 40, 5), (384, 200, 3)):  # (the oracle's gelu leaves a tail of size % 8 untouched, as the reference does)
        x, g, b, W = _decoder_like(r, B, K, N, DT_F32, scale=1.0 / np.sqrt(K))
        bias = (0.1 * r.standard_normal(N)).astype(np.float32)
        res = r.standard_normal((B, N)).astype(np.float32)
        a = oracle.layer_norm(x, g, b)
        pre = oracle.matmul(a, W, bias)
        scale = np.abs(a.astype(np.float64)) @ np.abs(W.astype(np.float64)).T + np.abs(bias)
        ref, _ = linear_ref(x, W, bias, DT_F32, ln=(g, b))
        assert (np.abs(ref - pre) <= 2e-5 * scale).all()
        for mode in (0, 1):
            ref, _ = linear_ref(x, W, bias, DT_F32, ln=(g, b), act=True, gelu_mode=mode, residual=res)
            assert (np.abs(ref - (oracle.gelu(pre, mode).astype(np.float64) + res)) <= 3e-5 * (scale + 1)).all()
        ref, _ = linear_ref(x, W, bias, DT_F32, residual=res)  # no LayerNorm
        assert (np.abs(ref - (oracle.matmul(x, W, bias).astype(np.float64) + res)) <= 2e-5 * (np.abs(x) @ np.abs(W).T + 3)).all()
    z = np.linspace(-6, 6, 1000)
    for mode in (0, 1):  # gelu64's derivative is the derivative of its value
        g0, gp, _, _ = gelu64(z, mode)
        h = 1e-6
        num = (gelu64(z + h, mode)[0] - gelu64(z - h, mode)[0]) / (2 * h)
        assert np.abs(num - gp).max() < 1e-8
        assert np.abs(g0 - oracle.gelu(z.astype(np.float32), mode)).max() < 2e-6


def test_prefill_row_mappings_equal_a_stepwise_loop():
    """Row -> (utterance, cache row) of the QKV prefill and row -> key count of the causal prefill against a plain per-utterance
    stepwise loop; the per-row-count attention reference equals the whole-cache reference on each row's own slice."""
    for P, n_utt, length in ((1, 3, 0), (4, 17, 2), (5, 2, 7)):
        rows = {}
        for b in range(n_utt):  # utterance by utterance, one position after the other
            cur = length
            for p in range(P):
                rows[p * n_utt + b] = (b, cur, cur + 1)  # appended at row cur; the query then sees cur + 1 keys
                cur += 1
        kvB = n_utt if P > 1 else 0
        assert qkv_scatter(P * n_utt, n_utt, kvB, length) == [rows[i][:2] for i in range(P * n_utt)]
        assert prefill_counts(P, n_utt, length) == [rows[i][2] for i in range(P * n_utt)]
    r = np.random.default_rng(3)
    P, q_B, length, H = 3, 2, 4, 2
    q = r.standard_normal((P * q_B, 64 * H)).astype(np.float32)
    k, v = r.standard_normal((2, q_B, 9, 64 * H)).astype(np.float32)
    counts = prefill_counts(P, q_B, length)
    got = attention_cached_ref(q, k, v, H, counts=counts, q_B=q_B)
    for row, n in enumerate(counts):
        u = row % q_B
        one = attention_cached_ref(q[row:row + 1], k[u:u + 1, :n], v[u:u + 1, :n], H)
        assert np.abs(one[0] - got[row]).max() < 1e-13  # (the whole-cache path sums through einsum: another float64 order)


def _emulate(x, W, bias, g, b, dt, nw, kpw, act, mode, drop_kstep=None, swap_group=None, bias_after=False, trunc=False, gamma_off=None):
    """numpy fp32 emulation of dec_linear_kernel's summation order for an (nw x kpw) split: per-lane sequential LayerNorm sums over
    its 8·kpw values, the two butterfly adds, the nw partials in wave order; LayerNorm output rounded to dt; per wave kpw chained
    32-wide MFMAs (exact products, one fp32 rounding per MFMA; fp32 operands: products rounded, eight 4-wide MFMAs per k-step), the
    nw partials added in wave order; bias, GELU.  drop_kstep / swap_group / bias_after: deliberate mistakes; trunc (the LayerNorm output
    truncated to dt instead of rounded to nearest) and gamma_off (one gamma element 1 % off) are the subtle ones."""
    f = np.float32
    B, K = x.shape
    w = _round(W, dt)
    out = np.zeros((B, W.shape[0]))
    ksteps = [[(wv + nw * i) * 32 for i in range(kpw)] for wv in range(nw)]
    for r in range(B):
        sm_w, sq_w = [], []
        for wv in range(nw):
            lane_s, lane_q = [], []
            for grp in range(4):
                s = q = f(0)
                for k0 in ksteps[wv]:
                    for j in range(8):
                        val = x[r, k0 + grp * 8 + j]
                        s = f(s + val)
                        q = f(q + f(val * val))
                lane_s.append(s)
                lane_q.append(q)
            sm_w.append(f(f(lane_s[0] + lane_s[1]) + f(lane_s[2] + lane_s[3])))
            sq_w.append(f(f(lane_q[0] + lane_q[1]) + f(lane_q[2] + lane_q[3])))
        sm = sq = f(0)
        for wv in range(nw):
            sm, sq = f(sm + sm_w[wv]), f(sq + sq_w[wv])
        mean = f(sm / f(K))
        var = f(f(sq / f(K)) - f(mean * mean))
        rstd = f(f(1) / np.sqrt(f(var + f(1e-5))))
        gg, bb = g.copy(), b.copy()
        if gamma_off is not None:
            gg[gamma_off] *= f(1.01)
        if swap_group is not None:
            sl = slice(swap_group * 8, swap_group * 8 + 8)
            gg[sl], bb[sl] = b[sl], g[sl]
        a = ((((x[r] - mean).astype(f) * rstd).astype(f) * gg).astype(f) + bb).astype(f)
        at = _round(a, dt)
        if trunc and dt != DT_F32:
            up = np.abs(at) > np.abs(a)
            at = np.where(up, at - np.sign(at) * _ulp_tw(at, dt)[1] * np.where(np.frexp(np.abs(at))[0] == 0.5, 1, 2), at)
        acc = np.zeros(W.shape[0], f)
        for wv in range(nw):
            part = np.zeros(W.shape[0], f)
            for k0 in ksteps[wv]:
                if drop_kstep == k0 // 32:
                    continue
                if dt == DT_F32:
                    for k4 in range(k0, k0 + 32, 4):
                        part = (part + (w[:, k4:k4 + 4] * at[k4:k4 + 4]).astype(f).astype(np.float64).sum(1)).astype(f)
                else:
                    part = (part + (w[:, k0:k0 + 32] * at[k0:k0 + 32]).sum(1)).astype(f)
            acc = part if wv == 0 else (acc + part).astype(f)
        z = acc if bias_after else (acc + bias).astype(f)
        if act:
            z = gelu64(z.astype(np.float64), mode)[0].astype(f)
        if bias_after:
            z = (z + bias).astype(f)
        out[r] = z
    return out


def test_summation_order_emulation_inside_bound_and_mistakes_outside():
    """A numpy fp32 emulation of the kernel's summation order stays INSIDE linear_ref's bound for one case per dtype, and three
    deliberately wrong emulations (one k-step dropped; gamma and beta swapped for one 8-column group; bias added after GELU) and
    two subtle ones (one gamma element 1 % off; the 16-bit operand conversion truncating instead of rounding to nearest) fall
    OUTSIDE it: the bound is tight enough to be worth running on the GPU."""
    for dt, K, nw, kpw in ((DT_BF16, 384, 4, 3), (DT_F16, 128, 2, 2), (DT_F32, 128, 4, 1)):
        r = np.random.default_rng(K + dt)
        B, N = 6, 48
        x, g, b, W = _decoder_like(r, B, K, N, dt, scale=1.0 / np.sqrt(K))
        bias = (0.1 * r.standard_normal(N)).astype(np.float32)
        for mode in (0, 1):
            ref, bound = linear_ref(x, W, bias, dt, ln=(g, b), act=True, gelu_mode=mode, depth=ln_depth((nw, kpw)))
            ok = _emulate(x, W, bias, g, b, dt, nw, kpw, True, mode)
            ratio = (np.abs(ok - ref) / bound).max()
            print(f"dt {dt} K {K} gelu {mode}: emulation worst err/bound {ratio:.3g}")
            assert ratio <= 1.0
            rt, bt = store16(ref, bound, dt)  # the 16-bit store of the same values
            assert (np.abs(_round(ok, dt) - rt) <= bt).all()
            for wrong in (dict(drop_kstep=1), dict(swap_group=5), dict(bias_after=True), dict(gamma_off=int(np.argmax(np.abs(x[0])))),) + \
                    ((dict(trunc=True),) if dt != DT_F32 else ()):
                bad = _emulate(x, W, bias, g, b, dt, nw, kpw, True, mode, **wrong)
                worst = (np.abs(bad - ref) / bound).max()
                assert worst > 1.0, (dt, mode, wrong, worst)
                if dt != DT_F32:
                    assert (np.abs(_round(bad, dt) - rt) > bt).any(), (dt, mode, wrong)
