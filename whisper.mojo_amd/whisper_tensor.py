"""Host-side mirror of /root/reference/whisper_tensor.mojo: the op functions with the reference's names and
argument meaning (out-param first), each a thin call through the C-ABI into a HIP kernel.  `Tensor` is a
row-major fp32 numpy array [rows, cols] (whisper_tensor.mojo:10-15)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .config import DT_BF16, DT_F32, GELU_TANH


def Tensor(rows: int, cols: int) -> np.ndarray:
    """whisper_tensor.mojo:17-23: zero-filled [rows, cols] fp32."""
    return np.zeros((rows, cols), np.float32)


def _fp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def _chk_out(out, shape):
    if out.dtype != np.float32 or not out.flags.c_contiguous or out.shape != tuple(shape):
        raise ValueError(f"out must be a C-contiguous float32 array of shape {tuple(shape)}")


def matmul(C_out: np.ndarray, A, B, bias=None, dtype=DT_F32):
    """whisper_tensor.mojo:151-246: C = A·Bᵀ (+bias); B in HF [out,in] layout."""
    A, B = np.ascontiguousarray(A, np.float32), np.ascontiguousarray(B, np.float32)
    b = None if bias is None or bias.size == 0 else np.ascontiguousarray(bias, np.float32).ravel()
    M, K = A.shape
    N = B.shape[0]
    _chk_out(C_out, (M, N))
    _lib.check(_lib.lib().wm_op_matmul_nt(_fp(C_out), _fp(A), _fp(B), _fp(b), M, N, K, dtype))


def ln_matmul(C_out: np.ndarray, A, ln_g, ln_b, B, bias=None, dtype=DT_F32, require_fused: bool = False):
    """layers.mojo:449-455 / 489-497: C = layer_norm(A)·Bᵀ (+bias).  require_fused: demand the one-kernel form (the LayerNorm applied
    while the GEMM loads A); a shape that kernel does not take raises (WM_E_ARG) and leaves C_out untouched."""
    f = lambda a: np.ascontiguousarray(a, np.float32)
    A, B, ln_g, ln_b = f(A), f(B), f(ln_g).ravel(), f(ln_b).ravel()
    b = None if bias is None or bias.size == 0 else f(bias).ravel()
    M, K = A.shape
    N = B.shape[0]
    _chk_out(C_out, (M, N))
    _lib.check(_lib.lib().wm_op_ln_matmul_nt(_fp(C_out), _fp(A), _fp(ln_g), _fp(ln_b), _fp(B), _fp(b), M, N, K, dtype, int(require_fused)))


def mlp_block(x: np.ndarray, ln_g, ln_b, fc1_w, fc1_b, fc2_w, fc2_b, next_ln=None, dtype=DT_F32, gelu_mode: int = GELU_TANH):
    """layers.mojo:489-517 (the MLP half of ResidualAttentionBlock.forward): x += fc2(gelu(fc1(layer_norm(x)))), in place.
    next_ln = (gamma, beta): also returns layer_norm(x_new) rounded to the operand dtype — the rows the next projection reads."""
    _chk_out(x, x.shape)
    M, d = x.shape
    f = lambda a: np.ascontiguousarray(a, np.float32)
    ln_g, ln_b, fc1_w, fc1_b, fc2_w, fc2_b = f(ln_g).ravel(), f(ln_b).ravel(), f(fc1_w), f(fc1_b).ravel(), f(fc2_w), f(fc2_b).ravel()
    ffn = fc1_w.shape[0]
    if fc1_w.shape != (ffn, d) or fc2_w.shape != (d, ffn):
        raise ValueError("fc1_w must be [ffn, d] and fc2_w [d, ffn]")
    ng = nb = xn = None
    if next_ln is not None:
        ng, nb = f(next_ln[0]).ravel(), f(next_ln[1]).ravel()
        xn = np.empty((M, d), np.float32)
    _lib.check(_lib.lib().wm_op_mlp_block(_fp(x), _fp(ln_g), _fp(ln_b), _fp(fc1_w), _fp(fc1_b), _fp(fc2_w), _fp(fc2_b), _fp(ng), _fp(nb),
                                          _fp(xn), M, d, ffn, dtype, gelu_mode))
    return xn


def attention(out: np.ndarray, q, k, v, n_heads: int, dtype=DT_F32):
    """layers.mojo:273-342, the block path without cache or mask (the encoder's): per head softmax(q_h·k_hᵀ / 8)·v_h."""
    f = lambda a: np.ascontiguousarray(a, np.float32)
    q, k, v = f(q), f(k), f(v)
    n_ctx, d = q.shape
    if d != 64 * n_heads or k.shape != q.shape or v.shape != q.shape:
        raise ValueError("q, k, v must be [n_ctx, 64 * n_heads]")
    _chk_out(out, q.shape)
    _lib.check(_lib.lib().wm_op_attention(_fp(out), _fp(q), _fp(k), _fp(v), n_ctx, n_heads, dtype))


def attention_batch(out: np.ndarray, q, k, v, n_heads: int, dtype=DT_F32):
    """attention over B utterances in one launch (wm_op_attention_batch): q, k, v, out [B, n_ctx, 64 * n_heads]."""
    f = lambda a: np.ascontiguousarray(a, np.float32)
    q, k, v = f(q), f(k), f(v)
    if q.ndim != 3 or q.shape[2] != 64 * n_heads or k.shape != q.shape or v.shape != q.shape:
        raise ValueError("q, k, v must be [B, n_ctx, 64 * n_heads]")
    _chk_out(out, q.shape)
    _lib.check(_lib.lib().wm_op_attention_batch(_fp(out), _fp(q), _fp(k), _fp(v), q.shape[0], q.shape[1], n_heads, dtype))


def attention_cached(out: np.ndarray, q, k, v, n_heads: int, kv_dtype=DT_F32, n_chunks: int = 1, out_dtype=DT_F32, q_B: int = 0,
                     len: int = -1, nq: int = 0, key_lo=None):
    """layers.mojo:186-272, the q_len == 1 path over cached rows: q [B, d], k / v [B, t, d] -> out [B, d].
    key_lo [B (or q_B)] (n_chunks == 1; wm_op_attention_cached_lo): utterance u sweeps rows [key_lo[u], len + 1 (+ p)) only; an empty
    window gives zeros.
    n_chunks > 1: the cross-attention form (keys swept by several workgroups and merged).  out_dtype: what the kernels store
    (returned widened).  len >= 0 (n_chunks == 1): a row sweeps len + 1 of the t rows.  q_B > 0: prefill, q [P·q_B, d] position-major,
    k / v [q_B, t, d]: row p·q_B + b attends over utterance b (n_chunks == 1: its first len + 1 + p rows).  nq = 4: the chunked
    prefill form that serves four positions from one sweep."""
    f = lambda a: np.ascontiguousarray(a, np.float32)
    q, k, v = f(q), f(k), f(v)
    B, d = q.shape
    n_utt = q_B if q_B > 0 else B
    if d != 64 * n_heads or k.ndim != 3 or k.shape[0] != n_utt or k.shape[2] != d or v.shape != k.shape:
        raise ValueError("q must be [B, 64 * n_heads], k and v [B (or q_B), t, 64 * n_heads]")
    if q_B > 0 and B % q_B:
        raise ValueError("prefill rows are position-major: q must be [P * q_B, d]")
    _chk_out(out, q.shape)
    if key_lo is not None:
        lo = np.ascontiguousarray(np.asarray(key_lo, np.int32).reshape(-1))
        if lo.size != n_utt:
            raise ValueError(f"key_lo needs one entry per utterance ({n_utt})")
        _lib.check(_lib.lib().wm_op_attention_cached_lo(_fp(out), _fp(q), _fp(k), _fp(v), B, k.shape[1], n_heads, kv_dtype, n_chunks,
                                                        out_dtype, q_B, len, nq, lo.ctypes.data_as(C.POINTER(C.c_int32))))
        return
    _lib.check(_lib.lib().wm_op_attention_cached(_fp(out), _fp(q), _fp(k), _fp(v), B, k.shape[1], n_heads, kv_dtype, n_chunks, out_dtype,
                                                 q_B, len, nq))


def _utt_map(utt_of, n_slots):
    m = np.ascontiguousarray(np.asarray(utt_of, np.int32).reshape(-1))
    if m.size != n_slots:
        raise ValueError(f"utt_of needs one entry per batch slot ({n_slots}), got {m.size}")
    return m


def attention_cached_map(out: np.ndarray, q, k, v, utt_of, n_heads: int, kv_dtype=DT_F32, n_chunks: int = 2, out_dtype=DT_F32,
                         q_B: int = 0, nq: int = 0):
    """attention_cached's chunked forms (n_chunks >= 2) with K/V by row map (wm_op_attention_cached_map): k / v
    [n_utt, t, d], utt_of [q_B, or B when q_B == 0]: the query row in batch slot b attends over clip utt_of[b]."""
    f = lambda a: np.ascontiguousarray(a, np.float32)
    q, k, v = f(q), f(k), f(v)
    if q.ndim != 2 or q.shape[1] != 64 * n_heads or k.ndim != 3 or k.shape[2] != q.shape[1] or v.shape != k.shape:
        raise ValueError("q must be [B, 64 * n_heads], k and v [n_utt, t, 64 * n_heads]")
    B = q.shape[0]
    if q_B < 0 or (q_B > 0 and B % q_B):
        raise ValueError("prefill rows are position-major: q must be [P * q_B, d]")
    if n_chunks < 2:
        raise ValueError("the map belongs to the chunked forms (n_chunks >= 2)")
    m = _utt_map(utt_of, q_B if q_B > 0 else B)
    _chk_out(out, q.shape)
    _lib.check(_lib.lib().wm_op_attention_cached_map(_fp(out), _fp(q), _fp(k), _fp(v), B, k.shape[1], n_heads, kv_dtype, n_chunks, out_dtype,
                                                     q_B, -1, nq, m.ctypes.data_as(C.POINTER(C.c_int32)), k.shape[0]))


def dec_linear(x, W, bias=None, ln=None, residual=None, in_place: bool = False, dtype=DT_F32, x_is_t: bool = False, out_is_t: bool = False,
               act: bool = False, gelu_mode: int = GELU_TANH, kv=None, kv_dtype=DT_F32, kv_B: int = 0, len: int = 0, cap=None,
               cap_sel=None, cap_step0: int = 0, _hook: str = "wm_op_dec_linear"):
    """One launch of the decode step's skinny linear (wm_op_dec_linear): epi(pro(x)·Wᵀ + bias) -> out [B, N] fp32.
    ln = (gamma, beta): LayerNorm prologue; x_is_t: x goes up in operand dtype; act: GELU; residual [B, N] is added (in_place: through
    the aliasing form, out = residual buffer); out_is_t: the kernel stores operand dtype.  kv = (kcache, vcache) [n_utt, cap_rows, d]
    with N = 3·d: QKV mode, returns (q [B, d], kcache, vcache) — the caches as they stand after the append at row len (kv_B > 0:
    prefill rows, position-major).  cap [B, cap_steps, cap_nsel, 64] with cap_sel [32]: alignment-head capture, returns (out, cap)."""
    f = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    x, W, bias, residual = f(x), f(W), f(bias), f(residual)
    if x.ndim != 2 or W.ndim != 2 or W.shape[1] != x.shape[1]:
        raise ValueError("x must be [B, K] and W [N, K]")
    B, K = x.shape
    N = W.shape[0]
    if bias is not None and bias.size != N:
        raise ValueError("bias must have N elements")
    g = b = None
    if ln is not None:
        g, b = f(ln[0]).ravel(), f(ln[1]).ravel()
        if g.size != K or b.size != K:
            raise ValueError("ln gamma / beta must have K elements")
    if residual is not None and residual.shape != (B, N):
        raise ValueError("residual must be [B, N]")
    kc = vc = None
    n_utt = cap_rows = 0
    wout = N
    if kv is not None:
        kc, vc = f(kv[0]).copy(), f(kv[1]).copy()
        if N % 3 or kc.ndim != 3 or kc.shape[2] != N // 3 or vc.shape != kc.shape:
            raise ValueError("QKV mode: W must be [3 * d, K] and kcache / vcache [n_utt, cap_rows, d]")
        n_utt, cap_rows, wout = kc.shape
    cp = sel = None
    steps = nsel = 0
    if cap is not None:
        cp = f(cap).copy()
        sel = np.ascontiguousarray(cap_sel, np.int8)
        if cp.ndim != 4 or cp.shape[0] != B or cp.shape[3] != 64 or sel.shape != (32,):
            raise ValueError("cap must be [B, cap_steps, cap_nsel, 64] and cap_sel [32]")
        steps, nsel = cp.shape[1], cp.shape[2]
    out = np.zeros((B, wout), np.float32)
    res = residual
    if residual is not None and in_place:
        out[:] = residual
        res = out
    _lib.check(getattr(_lib.lib(), _hook)(_fp(out), _fp(x), _fp(W), _fp(bias), _fp(g), _fp(b), _fp(res), B, N, K, dtype, int(x_is_t),
                                          int(out_is_t), int(act), gelu_mode, _fp(kc), _fp(vc), n_utt, cap_rows, kv_dtype, kv_B, len,
                                          _fp(cp), None if sel is None else sel.ctypes.data_as(C.POINTER(C.c_int8)), cap_step0, steps,
                                          nsel))
    if kv is not None:
        return out, kc, vc
    if cap is not None:
        return out, cp
    return out


def dec_linear_long(x, W, bias=None, **kw):
    """dec_linear on the K-long form of the kernel (wm_op_dec_linear_long): 16 waves walking groups of k-steps, K = 3072 or 4096 (fc2
    of d_model 768 / 1024), no LayerNorm prologue.  Arguments and results as dec_linear's."""
    return dec_linear(x, W, bias, _hook="wm_op_dec_linear_long", **kw)


def layer_norm(out: np.ndarray, inp, gamma, beta, eps: float = 1e-5):
    """whisper_tensor.mojo:249-285"""
    x = np.ascontiguousarray(inp, np.float32)
    g, b = np.ascontiguousarray(gamma, np.float32).ravel(), np.ascontiguousarray(beta, np.float32).ravel()
    _chk_out(out, x.shape)
    _lib.check(_lib.lib().wm_op_layer_norm(_fp(out), _fp(x), _fp(g), _fp(b), x.shape[0], x.shape[1], eps))


def layer_norm_t(inp, gamma, beta, eps: float = 1e-5, dtype=DT_F32, out_t=None, out_f=None):
    """One launch of the LayerNorm kernel with its operand-dtype store (out_t, returned widened to fp32), its fp32 store (out_f), or
    both (wm_op_layer_norm_t).  out_t / out_f: caller's [rows + 1, cols] float32 arrays, at least one, in and out: rows the kernel does not
    write (the guard row after the last) keep the caller's values."""
    x = np.ascontiguousarray(inp, np.float32)
    g, b = np.ascontiguousarray(gamma, np.float32).ravel(), np.ascontiguousarray(beta, np.float32).ravel()
    if out_t is None and out_f is None:
        raise ValueError("out_t, out_f or both")
    for o in (out_t, out_f):
        if o is not None:
            _chk_out(o, (x.shape[0] + 1, x.shape[1]))
    _lib.check(_lib.lib().wm_op_layer_norm_t(_fp(out_t), _fp(out_f), _fp(x), _fp(g), _fp(b), x.shape[0], x.shape[1], eps, dtype))


GEMM_NT_KERNELS = {-1: "refused", 0: "direct", 1: "lds", 2: "rowpanel", 3: "fullrow"}  # whisper_mi.h WM_GEMM_NT_*


def gemm_nt_epi(C_flat: np.ndarray, A_flat, W, M, lda=None, batch=1, strideA=0, ldc=None, strideC=0, bias=None, pos=None, residual=None,
                ldr=0, strideR=0, residual_in_place=False, act=False, gelu_mode: int = GELU_TANH, group_n=0, group_stride=0, dtype=DT_F32,
                out_dtype=DT_F32) -> str:
    """One launch of the encoder's tiled GEMM with its whole epilogue (wm_op_gemm_nt_epi, whisper_mi.h): C_flat is the caller's flat
    float32 array, in and out (cells the kernel does not write keep their values); A_flat a flat array of (batch-1)·strideA +
    (M-1)·lda + K elements; W [N, K].  -> the kernel that ran, a name of GEMM_NT_KERNELS."""
    f = lambda a: None if a is None else np.ascontiguousarray(a, np.float32).ravel()
    W = np.ascontiguousarray(W, np.float32)
    N, K = W.shape
    A_flat, bias, pos, residual = f(A_flat), f(bias), f(pos), f(residual)
    _chk_out(C_flat, (C_flat.size,))
    if bias is not None and bias.size != N:
        raise ValueError("bias must have N elements")
    if pos is not None and pos.size != M * N:
        raise ValueError("pos must be [M, N]")
    ran = C.c_int32(-1)
    _lib.check(_lib.lib().wm_op_gemm_nt_epi(_fp(C_flat), C_flat.size, _fp(A_flat), A_flat.size, _fp(W), _fp(bias), _fp(pos), _fp(residual),
                                            0 if residual is None else residual.size, M, N, K, batch, K if lda is None else lda, strideA,
                                            N if ldc is None else ldc, strideC, ldr, strideR, int(bool(residual_in_place)), int(bool(act)),
                                            gelu_mode, group_n, group_stride, dtype, out_dtype, C.byref(ran)))
    return GEMM_NT_KERNELS[ran.value]


def gemm_nt_ring(C_flat: np.ndarray, A_flat, W, M, lda=None, batch=1, strideA=0, ldc=None, strideC=0, bias=None, pos=None, residual=None,
                 ldr=0, strideR=0, residual_in_place=False, act=False, gelu_mode: int = GELU_TANH, group_n=0, group_stride=0, dtype=DT_BF16,
                 out_dtype=DT_F32, ln=None, lno=None, lno_out=None) -> str:
    """gemm_nt_epi for the shapes that run on the encoder's row-panel and full-row kernels (wm_op_gemm_nt_ring, whisper_mi.h).  ln =
    (gamma [K], beta [K]): A_flat holds fp32 residual rows which the row-panel kernel normalises while loading.  lno = (gamma [N],
    beta [N]) with lno_out, the caller's flat float32 array laid out like C_flat, in and out: the full-row kernel's 16-bit LayerNorm
    rows, widened.  -> the kernel that ran."""
    f = lambda a: None if a is None else np.ascontiguousarray(a, np.float32).ravel()
    W = np.ascontiguousarray(W, np.float32)
    N, K = W.shape
    A_flat, bias, pos, residual = f(A_flat), f(bias), f(pos), f(residual)
    _chk_out(C_flat, (C_flat.size,))
    if bias is not None and bias.size != N:
        raise ValueError("bias must have N elements")
    if pos is not None and pos.size != M * N:
        raise ValueError("pos must be [M, N]")
    ln_g, ln_b = (None, None) if ln is None else (f(ln[0]), f(ln[1]))
    lno_g, lno_b = (None, None) if lno is None else (f(lno[0]), f(lno[1]))
    if ln is not None and (ln_g.size != K or ln_b.size != K):
        raise ValueError("ln gamma / beta must have K elements")
    if lno is not None and (lno_g.size != N or lno_b.size != N):
        raise ValueError("lno gamma / beta must have N elements")
    if (lno is None) != (lno_out is None):
        raise ValueError("lno and lno_out go together")
    if lno_out is not None:
        _chk_out(lno_out, (lno_out.size,))
    ran = C.c_int32(-1)
    _lib.check(_lib.lib().wm_op_gemm_nt_ring(_fp(C_flat), C_flat.size, _fp(A_flat), A_flat.size, _fp(W), _fp(bias), _fp(pos), _fp(residual),
                                             0 if residual is None else residual.size, M, N, K, batch, K if lda is None else lda, strideA,
                                             N if ldc is None else ldc, strideC, ldr, strideR, int(bool(residual_in_place)), int(bool(act)),
                                             gelu_mode, group_n, group_stride, dtype, out_dtype, _fp(ln_g), _fp(ln_b), _fp(lno_g), _fp(lno_b),
                                             _fp(lno_out), 0 if lno_out is None else lno_out.size, C.byref(ran)))
    return GEMM_NT_KERNELS[ran.value]


def gelu(t: np.ndarray, mode: int = GELU_TANH):
    """whisper_tensor.mojo:288-308 — in place."""
    _chk_out(t, t.shape)
    _lib.check(_lib.lib().wm_op_gelu(_fp(t), t.size, mode))


def softmax(t: np.ndarray):
    """whisper_tensor.mojo:311-355 — rows, in place."""
    _chk_out(t, t.shape)
    _lib.check(_lib.lib().wm_op_softmax_rows(_fp(t), t.shape[0], t.shape[1]))


def conv1d(out: np.ndarray, inp, weight, bias, stride: int, padding: int = 1, out_T: bool = False, dtype=DT_F32):
    """whisper_tensor.mojo:367-428 (K=3).  `weight` is the file-layout [C_out, C_in, 3] tensor; the reference's
    transpose_conv_weights (:358-364) re-layout happens inside the library."""
    if padding != 1:
        raise ValueError("the reference only ever uses padding=1 (whisper.mojo:74,79)")
    x, w = np.ascontiguousarray(inp, np.float32), np.ascontiguousarray(weight, np.float32)
    b = np.ascontiguousarray(bias, np.float32).ravel()
    C_in, L_in = x.shape
    C_out = w.shape[0]
    L_out = (L_in + 2 - 3) // stride + 1
    _chk_out(out, (L_out, C_out) if out_T else (C_out, L_out))
    _lib.check(_lib.lib().wm_op_conv1d_k3(_fp(out), _fp(x), _fp(w), _fp(b), C_in, L_in, C_out, stride, int(out_T), dtype))


def argmax(t) -> int:
    """whisper_tensor.mojo:431-439: lowest index wins ties."""
    x = np.ascontiguousarray(t, np.float32).ravel()
    idx = C.c_int32(0)
    _lib.check(_lib.lib().wm_op_argmax(_fp(x), x.size, C.byref(idx)))
    return int(idx.value)


def logits_argmax(x, ln_g, ln_b, emb, dtype=DT_F32, mask=None, ranges=None, timestamp_begin: int = 0, return_logprobs: bool = False,
                  seen=None, ban=None, penalty: float = 1.0, hit=None, slot_id=None, slot_bias=None, slot_flags=None):
    """whisper.mojo:156-166 + the greedy argmax: (logits [B, N] = layer_norm(x)·embᵀ, ids [B]) on the decode step's logits kernel
    and fused argmax.  mask [N] additive (0 / -inf) on the argmax candidates; ranges [B, 4] = (text_lo, text_hi, ts_lo, ts_hi)
    with timestamp_begin > 0: the timestamp decision (wm_op_logits).  return_logprobs: (logits, ids, logprob [B]) from the log-prob
    instantiation of the same kernels (wm_op_logits_lp): logits[id] - logsumexp over the candidates the mask and the ranges leave.
    seen / ban [B, ceil(N / 32)] uint32 (both or neither): the repetition-processor instantiation (wm_op_logits_processed, DESIGN
    §29) — row b's logits at the ids of seen[b] times (negative) or over (else) `penalty`, those of ban[b] -inf, ahead of all of the
    above; the returned logits are the processed ones.  hit [B, ceil(N / 32)] uint32 with slot_id [S] (ascending ids), slot_bias
    [B, S] float32 and slot_flags [B, S] int32 (bit 0 on, bit 1 ban), beside seen / ban: the sequence-bias instantiation
    (wm_op_logits_seq_bias) — where row b's hit bit of an id is set its slot's bias is added ahead of the penalty, or the
    value is -inf under a ban."""
    f = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    x, emb, mask = f(x), f(emb), f(mask)
    g, b = f(ln_g).ravel(), f(ln_b).ravel()
    if x.ndim != 2 or emb.ndim != 2 or emb.shape[1] != x.shape[1] or g.size != x.shape[1] or b.size != x.shape[1]:
        raise ValueError("x must be [B, K], emb [N, K], ln_g / ln_b [K]")
    B, K = x.shape
    N = emb.shape[0]
    if mask is not None and mask.size != N:
        raise ValueError("mask must have N elements")
    rg = None
    if ranges is not None:
        rg = np.ascontiguousarray(ranges, np.int32)
        if rg.shape != (B, 4):
            raise ValueError("ranges must be [B, 4]")
    logits = np.zeros((B, N), np.float32)
    ids = np.zeros(B, np.int32)
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    if seen is not None or ban is not None:
        words = (N + 31) // 32
        sets = [np.ascontiguousarray(a, np.uint32) for a in (seen, ban) if a is not None]
        if len(sets) != 2 or any(a.shape != (B, words) for a in sets):
            raise ValueError("seen and ban must both be [B, ceil(N / 32)] uint32")
        up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
        lp = np.zeros(B, np.float32) if return_logprobs else None
        if hit is not None:
            hw = np.ascontiguousarray(hit, np.uint32)
            sid = np.ascontiguousarray(slot_id, np.int32).ravel()
            sbias, sflags = np.ascontiguousarray(slot_bias, np.float32), np.ascontiguousarray(slot_flags, np.int32)
            if hw.shape != (B, words) or sbias.shape != (B, sid.size) or sflags.shape != (B, sid.size):
                raise ValueError("hit must be [B, ceil(N / 32)], slot_bias and slot_flags [B, len(slot_id)]")
            _lib.check(_lib.lib().wm_op_logits_seq_bias(_fp(logits), ip(ids), _fp(lp), _fp(x), _fp(g), _fp(b), _fp(emb),
                                                        _fp(mask.ravel() if mask is not None else None), ip(rg), int(timestamp_begin),
                                                        up(sets[0]), up(sets[1]), float(penalty), up(hw), ip(sid), int(sid.size), _fp(sbias),
                                                        ip(sflags), B, N, K, dtype))
            return (logits, ids, lp) if return_logprobs else (logits, ids)
        _lib.check(_lib.lib().wm_op_logits_processed(_fp(logits), ip(ids), _fp(lp), _fp(x), _fp(g), _fp(b), _fp(emb),
                                                     _fp(mask.ravel() if mask is not None else None), ip(rg), int(timestamp_begin),
                                                     up(sets[0]), up(sets[1]), float(penalty), B, N, K, dtype))
        return (logits, ids, lp) if return_logprobs else (logits, ids)
    if return_logprobs:
        lp = np.zeros(B, np.float32)
        _lib.check(_lib.lib().wm_op_logits_lp(_fp(logits), ip(ids), _fp(lp), _fp(x), _fp(g), _fp(b), _fp(emb),
                                              _fp(mask.ravel() if mask is not None else None), ip(rg), int(timestamp_begin), B, N, K, dtype))
        return logits, ids, lp
    _lib.check(_lib.lib().wm_op_logits(_fp(logits), ip(ids), _fp(x), _fp(g), _fp(b), _fp(emb), _fp(mask.ravel() if mask is not None else None),
                                       ip(rg), int(timestamp_begin), B, N, K, dtype))
    return logits, ids


def logits_topk(x, ln_g, ln_b, emb, k, dtype=DT_F32, mask=None, ranges=None, timestamp_begin: int = 0, seen=None, ban=None,
                penalty: float = 1.0):
    """logits_argmax(return_logprobs=True) with the top-k alternatives (wm_op_logits_topk): (logits [B, N], ids [B],
    logprob [B], top_ids [B, k] int32, top_logprobs [B, k] float32) from the decode step's logits kernel, the top-k instantiation of
    its arg-max launch and the selection launch behind it.  Per row the k candidates the mask and the ranges leave with the largest
    logit, descending, equal logits lowest id first, each with logit - logsumexp over those candidates (a forced timestamp: over the
    admissible timestamps alone); rank 0 equals (ids, logprob); a rank with no finite candidate left holds (-1, -inf).  mask, ranges,
    timestamp_begin, seen / ban / penalty: as logits_argmax.  1 <= k <= 8."""
    f = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    x, emb, mask = f(x), f(emb), f(mask)
    g, b = f(ln_g).ravel(), f(ln_b).ravel()
    if x.ndim != 2 or emb.ndim != 2 or emb.shape[1] != x.shape[1] or g.size != x.shape[1] or b.size != x.shape[1]:
        raise ValueError("x must be [B, K], emb [N, K], ln_g / ln_b [K]")
    B, K = x.shape
    N = emb.shape[0]
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= 8:
        raise ValueError("k must be an integer of [1, 8]")
    if mask is not None and mask.size != N:
        raise ValueError("mask must have N elements")
    rg = None
    if ranges is not None:
        rg = np.ascontiguousarray(ranges, np.int32)
        if rg.shape != (B, 4):
            raise ValueError("ranges must be [B, 4]")
    sets = [None, None]
    if seen is not None or ban is not None:
        sets = [np.ascontiguousarray(a, np.uint32) for a in (seen, ban) if a is not None]
        if len(sets) != 2 or any(a.shape != (B, (N + 31) // 32) for a in sets):
            raise ValueError("seen and ban must both be [B, ceil(N / 32)] uint32")
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    up = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint32))
    logits, ids, lp = np.zeros((B, N), np.float32), np.zeros(B, np.int32), np.zeros(B, np.float32)
    top_ids, top_lp = np.zeros((B, int(k)), np.int32), np.zeros((B, int(k)), np.float32)
    _lib.check(_lib.lib().wm_op_logits_topk(_fp(logits), ip(ids), _fp(lp), ip(top_ids), _fp(top_lp), int(k), _fp(x), _fp(g), _fp(b), _fp(emb),
                                            _fp(mask.ravel() if mask is not None else None), ip(rg), int(timestamp_begin), up(sets[0]),
                                            up(sets[1]), float(penalty), B, N, K, dtype))
    return logits, ids, lp, top_ids, top_lp


def score_logits(x, ln_g, ln_b, emb, target, dtype=DT_F32):
    """The score pass's vocabulary side alone (wm_op_score_logits): (logprob [M], top_id [M]) with logprob[r] =
    z[r][target[r]] - logsumexp(z[r]) over z = layer_norm(x)·embᵀ (0 where target[r] < 0) and top_id[r] = argmax z[r], lowest id on
    ties.  No logits matrix is formed."""
    f = lambda a: np.ascontiguousarray(a, np.float32)
    x, emb = f(x), f(emb)
    g, b = f(ln_g).ravel(), f(ln_b).ravel()
    tg = np.ascontiguousarray(target, np.int32).ravel()
    if x.ndim != 2 or emb.ndim != 2 or emb.shape[1] != x.shape[1] or g.size != x.shape[1] or b.size != x.shape[1] or tg.size != x.shape[0]:
        raise ValueError("x must be [M, K], emb [N, K], ln_g / ln_b [K], target [M]")
    if tg.max() >= emb.shape[0]:
        raise ValueError("a target is not a vocabulary id")
    M, K = x.shape
    lp, top = np.zeros(M, np.float32), np.zeros(M, np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    _lib.check(_lib.lib().wm_op_score_logits(_fp(lp), ip(top), _fp(x), _fp(g), _fp(b), _fp(emb), ip(tg), M, emb.shape[0], K, dtype))
    return lp, top


def no_speech(x, ln_g, ln_b, emb, token: int, dtype=DT_F32):
    """The no-speech probe's launches (wm_op_no_speech): (prob [B], lse [B]) — softmax(layer_norm(x)·embᵀ)[token] over
    all N columns (no mask, no ranges) and the row's logsumexp, on the kernel variant logits_argmax(return_logprobs=True) picks."""
    f = lambda a: np.ascontiguousarray(a, np.float32)
    x, emb = f(x), f(emb)
    g, b = f(ln_g).ravel(), f(ln_b).ravel()
    if x.ndim != 2 or emb.ndim != 2 or emb.shape[1] != x.shape[1] or g.size != x.shape[1] or b.size != x.shape[1]:
        raise ValueError("x must be [B, K], emb [N, K], ln_g / ln_b [K]")
    B, K = x.shape
    prob, lse = np.zeros(B, np.float32), np.zeros(B, np.float32)
    _lib.check(_lib.lib().wm_op_no_speech(_fp(prob), _fp(lse), _fp(x), _fp(g), _fp(b), _fp(emb), B, emb.shape[0], K, dtype, int(token)))
    return prob, lse


def lang_detect(x, ln_g, ln_b, emb, lang_ids, dtype=DT_F32):
    """lang_detect_kernel alone (wm_op_lang_detect): (ids [B], probs [B, n_lang]) — among lang_ids the id with the largest
    layer_norm(x)·emb[id] (ties: the smaller id) and the softmax over those candidates, in list order."""
    f = lambda a: np.ascontiguousarray(a, np.float32)
    x, emb = f(x), f(emb)
    g, b = f(ln_g).ravel(), f(ln_b).ravel()
    if x.ndim != 2 or emb.ndim != 2 or emb.shape[1] != x.shape[1] or g.size != x.shape[1] or b.size != x.shape[1]:
        raise ValueError("x must be [B, K], emb [N, K], ln_g / ln_b [K]")
    if x.shape[1] not in (128, 384, 512, 768, 1024):
        raise ValueError("K must be 128, 384, 512, 768 or 1024")
    ids = _lib.lang_args(lang_ids, emb.shape[0])
    B, K = x.shape
    out, probs = np.zeros(B, np.int32), np.zeros((B, ids.size), np.float32)
    _lib.check(_lib.lib().wm_op_lang_detect(out.ctypes.data_as(C.POINTER(C.c_int32)), _fp(probs), _fp(x), _fp(g), _fp(b), _fp(emb),
                                            ids.ctypes.data_as(C.POINTER(C.c_int32)), ids.size, B, emb.shape[0], K, dtype))
    return out, probs


def xattn(out: np.ndarray, q, Wk, Wv, bv, x, n_heads: int, nsplit: int, q_B: int = 0, out_dtype=DT_F32):
    """The absorbed cross-attention (wm_op_xattn): q [rows, d], Wk / Wv [d, d], bv [d], x [n_utt, n_keys, d], d = 64·n_heads;
    row r attends over x[r % q_B] (q_B > 0, prefill) or x[r] -> out [rows, d]."""
    f = lambda a: np.ascontiguousarray(a, np.float32)
    q, Wk, Wv, bv, x = f(q), f(Wk), f(Wv), f(bv).ravel(), f(x)
    d = 64 * n_heads
    if q.ndim != 2 or q.shape[1] != d or Wk.shape != (d, d) or Wv.shape != (d, d) or bv.size != d or x.ndim != 3 or x.shape[2] != d:
        raise ValueError("q must be [rows, 64 * n_heads], Wk / Wv [d, d], bv [d], x [n_utt, n_keys, d]")
    _chk_out(out, q.shape)
    _lib.check(_lib.lib().wm_op_xattn(_fp(out), _fp(q), _fp(Wk), _fp(Wv), _fp(bv), _fp(x), q.shape[0], q_B, x.shape[0], x.shape[1],
                                      n_heads, nsplit, out_dtype))


def xattn_map(out: np.ndarray, q, Wk, Wv, bv, x, utt_of, n_heads: int, nsplit: int, q_B: int = 0, out_dtype=DT_F32):
    """xattn with X by row map (wm_op_xattn_map): utt_of [q_B, or rows when q_B == 0]; the row in batch slot b attends
    over x[utt_of[b]]."""
    f = lambda a: np.ascontiguousarray(a, np.float32)
    q, Wk, Wv, bv, x = f(q), f(Wk), f(Wv), f(bv).ravel(), f(x)
    d = 64 * n_heads
    if q.ndim != 2 or q.shape[1] != d or Wk.shape != (d, d) or Wv.shape != (d, d) or bv.size != d or x.ndim != 3 or x.shape[2] != d:
        raise ValueError("q must be [rows, 64 * n_heads], Wk / Wv [d, d], bv [d], x [n_utt, n_keys, d]")
    if q_B < 0 or (q_B > 0 and q.shape[0] % q_B):
        raise ValueError("prefill rows are position-major: q must be [P * q_B, d]")
    m = _utt_map(utt_of, q_B if q_B > 0 else q.shape[0])
    _chk_out(out, q.shape)
    _lib.check(_lib.lib().wm_op_xattn_map(_fp(out), _fp(q), _fp(Wk), _fp(Wv), _fp(bv), _fp(x), q.shape[0], q_B, x.shape[0], x.shape[1],
                                          n_heads, nsplit, out_dtype, m.ctypes.data_as(C.POINTER(C.c_int32))))


def score_rank(key, n_cand):
    """The n-best ranking launch alone (wm_op_score_rank): key [R] fp32 grouped by clip, n_cand [U] >= 1 with
    sum n_cand = R -> (order [R] int32, best [U] int32, posterior [R] fp32)."""
    key = np.ascontiguousarray(np.asarray(key, np.float32).reshape(-1))
    n = np.ascontiguousarray(np.asarray(n_cand, np.int32).reshape(-1))
    if n.size < 1 or n.min() < 1 or int(n.sum()) != key.size:
        raise ValueError("n_cand needs one count >= 1 per clip, summing to the number of keys")
    order, best, post = np.full(key.size, -1, np.int32), np.full(n.size, -1, np.int32), np.zeros(key.size, np.float32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    _lib.check(_lib.lib().wm_op_score_rank(ip(order), ip(best), _fp(post), _fp(key), ip(n), n.size))
    return order, best, post


def xattn_absorb(q, Wk, n_heads: int, late_loads: bool = False) -> np.ndarray:
    """The absorb launch alone (wm_op_xattn_absorb): q [rows, d], Wk [d, d] -> the three bf16 images of q' [rows, 3, n_heads, d],
    widened to fp32.  late_loads: the loop that requests Wk after staging q; the same images bit for bit."""
    f = lambda a: np.ascontiguousarray(a, np.float32)
    q, Wk = f(q), f(Wk)
    d = 64 * n_heads
    if q.ndim != 2 or q.shape[1] != d or Wk.shape != (d, d):
        raise ValueError("q must be [rows, 64 * n_heads], Wk [d, d]")
    images = np.zeros((q.shape[0], 3, n_heads, d), np.float32)
    _lib.check(_lib.lib().wm_op_xattn_absorb(_fp(images), _fp(q), _fp(Wk), q.shape[0], n_heads, int(late_loads)))
    return images


def align_probs(q, layer_head_pairs, rows, n_layers: int, kv=None, kv_dtype=DT_F32, X=None, Wk=None, probs=None):
    """launch_align_probs alone (wm_op_align_probs): q [B, L, n_sel, 64] unscaled cross-q rows, layer_head_pairs [n_sel, 2], rows [B]
    (utterance b's first rows[b] <= L rows count).  Keys: kv [n_layers, 2, B, T, d] (the K/V cache, uploaded as kv_dtype) or the
    absorbed form X [B, T, d] + Wk [n_layers, 2, d, d] (uploaded as bf16).  probs [B, n_sel, L, T] in and out (None: zeros):
    softmax_j(0.125·q_r·K_j) in rows < rows[b], untouched elsewhere."""
    f = lambda a: np.ascontiguousarray(a, np.float32)
    q = f(q)
    pairs = np.ascontiguousarray(layer_head_pairs, np.int32)
    rows = np.ascontiguousarray(rows, np.int32).ravel()
    if q.ndim != 4 or q.shape[3] != 64 or pairs.ndim != 2 or pairs.shape != (q.shape[2], 2) or rows.size != q.shape[0]:
        raise ValueError("q must be [B, L, n_sel, 64], layer_head_pairs [n_sel, 2], rows [B]")
    B, L, n_sel, _ = q.shape
    if (kv is None) == (X is None and Wk is None) or (X is None) != (Wk is None):
        raise ValueError("keys: either kv, or X and Wk")
    if kv is not None:
        kv = f(kv)
        if kv.ndim != 5 or kv.shape[:3] != (n_layers, 2, B):
            raise ValueError("kv must be [n_layers, 2, B, T, d]")
        T, d = kv.shape[3:]
    else:
        X, Wk = f(X), f(Wk)
        if X.ndim != 3 or X.shape[0] != B or Wk.shape != (n_layers, 2, X.shape[2], X.shape[2]):
            raise ValueError("X must be [B, T, d], Wk [n_layers, 2, d, d]")
        T, d = X.shape[1:]
    if probs is None:
        probs = np.zeros((B, n_sel, L, T), np.float32)
    _chk_out(probs, (B, n_sel, L, T))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    _lib.check(_lib.lib().wm_op_align_probs(_fp(probs), _fp(q), _fp(kv), int(kv_dtype), _fp(X), _fp(Wk), ip(pairs), n_sel, ip(rows), B, L, T, d,
                                            int(n_layers)))
    return probs


def align_norm(weights, R, F, M=None):
    """launch_align_norm alone (wm_op_align_norm): weights [n_tab, n_sel, L, T], table b's R[b] x F[b] corner -> M [n_tab, L, T], in
    and out (None: zeros): z-score over the rows, width-7 reflect median over the columns, mean over the heads inside the corner,
    untouched elsewhere."""
    w = np.ascontiguousarray(weights, np.float32)
    R, F = np.ascontiguousarray(R, np.int32).ravel(), np.ascontiguousarray(F, np.int32).ravel()
    if w.ndim != 4 or R.size != w.shape[0] or F.size != w.shape[0]:
        raise ValueError("weights must be [n_tab, n_sel, L, T], R and F [n_tab]")
    n_tab, n_sel, L, T = w.shape
    if M is None:
        M = np.zeros((n_tab, L, T), np.float32)
    _chk_out(M, (n_tab, L, T))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    _lib.check(_lib.lib().wm_op_align_norm(_fp(M), _fp(w), n_tab, n_sel, L, T, ip(R), ip(F)))
    return M


def repeat_sets(tokens, prompt_len, n_ids, vocab: int, ngram: int, steps: int):
    """The repetition processors' bookkeeping alone (wm_op_repeat_sets): tokens [B, stride] int32, row b's prompt its first
    prompt_len[b] ids and its history n_ids[b] ids in all -> (seen, ban), each [steps + 1, B, ceil(vocab / 32)] uint32: entry 0 behind the
    init kernel, entry s behind the argmax launch that appended the row's id prompt_len[b] + s - 1 (a row past its end does nothing)."""
    tok = np.ascontiguousarray(tokens, np.int32)
    pl, nn = np.ascontiguousarray(prompt_len, np.int32).ravel(), np.ascontiguousarray(n_ids, np.int32).ravel()
    if tok.ndim != 2 or pl.size != tok.shape[0] or nn.size != tok.shape[0]:
        raise ValueError("tokens must be [B, stride], prompt_len and n_ids [B]")
    B, stride = tok.shape
    words = (vocab + 31) // 32
    seen = np.zeros((steps + 1, B, words), np.uint32)
    ban = np.zeros((steps + 1, B, words), np.uint32)
    ip, up = (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32)))
    _lib.check(_lib.lib().wm_op_repeat_sets(up(seen), up(ban), ip(tok), ip(pl), ip(nn), B, stride, int(vocab), int(ngram), int(steps)))
    return seen, ban


def seq_bias_hits(tokens, prompt_len, n_ids, vocab: int, sequence_bias, bad_words_ids, steps: int, eot: int = -1):
    """The sequence-bias bookkeeping alone (wm_op_seq_bias_hits): tokens / prompt_len / n_ids as repeat_sets, the two lists
    as transcribe_batch takes them -> (slot_id [S], hit [steps + 1, B, ceil(vocab / 32)] uint32, slot_bias [steps + 1, B, S] float32,
    slot_flags [steps + 1, B, S] int32): entry 0 behind the init kernel, entry s behind the argmax launch of step s."""
    tok = np.ascontiguousarray(tokens, np.int32)
    pl, nn = np.ascontiguousarray(prompt_len, np.int32).ravel(), np.ascontiguousarray(n_ids, np.int32).ravel()
    if tok.ndim != 2 or pl.size != tok.shape[0] or nn.size != tok.shape[0]:
        raise ValueError("tokens must be [B, stride], prompt_len and n_ids [B]")
    sb = _lib.seq_bias_args(sequence_bias, bad_words_ids, vocab)
    if sb is None:
        raise ValueError("both lists are empty")
    a = sb[1]
    B, stride = tok.shape
    words, cap = (vocab + 31) // 32, a[3] + a[6]
    hit = np.zeros((steps + 1, B, words), np.uint32)
    sbias, sflags = np.zeros((steps + 1, B, cap), np.float32), np.zeros((steps + 1, B, cap), np.int32)
    sid, ns = np.zeros(cap, np.int32), np.zeros(1, np.int32)
    ip, up = (lambda x: None if x is None else x.ctypes.data_as(C.POINTER(C.c_int32))), (lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32)))
    _lib.check(_lib.lib().wm_op_seq_bias_hits(up(hit), _fp(sbias), ip(sflags), ip(sid), ip(ns), ip(tok), ip(pl), ip(nn), B, stride, int(vocab),
                                              int(eot), ip(a[0]), ip(a[1]), _fp(a[2]), a[3], ip(a[4]), ip(a[5]), a[6], int(steps)))
    S = int(ns[0])
    return sid[:S].copy(), hit, sbias[:, :, :S].copy(), sflags[:, :, :S].copy()


def fe_tables(n_mels: int):
    """The front end's tables (wm_op_fe_tables, host only): (window [400], dft [512, 416], fb [201, n_mels], band [n_mels, 2])."""
    window, dft = np.zeros(400, np.float32), np.zeros((512, 416), np.float32)
    fb, band = np.zeros((201, max(1, int(n_mels))), np.float32), np.zeros((max(1, int(n_mels)), 2), np.int32)
    _lib.check(_lib.lib().wm_op_fe_tables(int(n_mels), _fp(window), _fp(dft), _fp(fb), band.ctypes.data_as(C.POINTER(C.c_int32))))
    return window, dft, fb, band


def fe_frames(pcm, n: int, t0: int = 0, n_samples=None, fill: float = 0.0):
    """frames_kernel alone (wm_op_fe_frames): pcm [B, N] -> (frames [B, n, 416] of frames t0 .. t0 + n, guard [416]); n_samples [B]:
    zero_tails_kernel runs first.  Everything starts as `fill`; guard is the row behind the last frame, which no kernel may store."""
    p = np.ascontiguousarray(pcm, np.float32)
    if p.ndim != 2:
        raise ValueError("pcm must be [B, N]")
    B, N = p.shape
    ns = None
    if n_samples is not None:
        ns = np.ascontiguousarray(np.asarray(n_samples, np.int32).reshape(-1))
        if ns.size != B:
            raise ValueError(f"n_samples needs one entry per row ({B})")
    out = np.full((B * max(0, int(n)) + 1, 416), fill, np.float32)
    _lib.check(_lib.lib().wm_op_fe_frames(_fp(out), _fp(p), None if ns is None else ns.ctypes.data_as(C.POINTER(C.c_int32)), B, N, int(n), int(t0)))
    return out[:-1].reshape(B, int(n), 416), out[-1]


def fe_mel_log(spec, n_mels: int, out_frames=None, t_out: int = 0, logmel=None):
    """mel_log_kernel alone (wm_op_fe_mel_log): spec [B, n, 512] -> logmel [B, n_mels, out_frames] (in and out; None: zeros), frames
    written at columns [t_out, t_out + n).  out_frames None: n."""
    s = np.ascontiguousarray(spec, np.float32)
    if s.ndim != 3 or s.shape[2] != 512:
        raise ValueError("spec must be [B, n, 512]")
    B, n, _ = s.shape
    F = n if out_frames is None else int(out_frames)
    if logmel is None:
        logmel = np.zeros((B, max(1, int(n_mels)), max(1, F)), np.float32)
    _chk_out(logmel, (B, max(1, int(n_mels)), max(1, F)))
    _lib.check(_lib.lib().wm_op_fe_mel_log(_fp(logmel), _fp(s), B, n, int(n_mels), F, int(t_out)))
    return logmel


def fe_mel_norm(logmel, long_mode: bool = False):
    """The clamp / rescale of the log-mel (wm_op_fe_mel_norm): rows [B, n] -> (max(x, rowmax - 8) + 4) / 4.  long_mode: the two-stage
    kernels of long audio, else mel_norm_kernel."""
    x = np.ascontiguousarray(logmel, np.float32)
    if x.ndim != 2:
        raise ValueError("logmel must be [B, n]")
    out = np.empty_like(x)
    _lib.check(_lib.lib().wm_op_fe_mel_norm(_fp(out), _fp(x), x.shape[0], x.shape[1], int(bool(long_mode))))
    return out


def window_gather(mel, items, W: int, fill: float = 0.0):
    """window_gather_kernel alone (wm_op_window_gather): mel [B, n_mels, F], items [(b, seek, len)] -> [rows, n_mels, W]; the output
    starts as `fill`, so a cell the kernel does not store shows."""
    m = np.ascontiguousarray(mel, np.float32)
    it = np.ascontiguousarray(np.asarray(items, np.int32).reshape(-1, 3))
    if m.ndim != 3:
        raise ValueError("mel must be [B, n_mels, F]")
    out = np.full((max(1, it.shape[0]), m.shape[1], max(1, int(W))), fill, np.float32)
    _lib.check(_lib.lib().wm_op_window_gather(_fp(out), _fp(m), it.ctypes.data_as(C.POINTER(C.c_int32)), it.shape[0], m.shape[0], m.shape[1],
                                              m.shape[2], int(W)))
    return out


def constraint_states(tokens, prompt_len, n_ids, vocab: int, phrases, steps: int, eot: int = -1, free_from=None, ngram: int = 0):
    """The phrase-list constraint's bookkeeping alone (wm_op_constraint_states): tokens / prompt_len / n_ids as
    repeat_sets, phrases as transcribe_batch's constraint= -> (node [steps + 1, B] int32, mask [steps + 1, B, ceil(vocab / 32)] uint32,
    the rows' ban words): entry 0 behind the init kernels, entry s behind the argmax launch of step s."""
    tok = np.ascontiguousarray(tokens, np.int32)
    pl, nn = np.ascontiguousarray(prompt_len, np.int32).ravel(), np.ascontiguousarray(n_ids, np.int32).ravel()
    if tok.ndim != 2 or pl.size != tok.shape[0] or nn.size != tok.shape[0]:
        raise ValueError("tokens must be [B, stride], prompt_len and n_ids [B]")
    ct = _lib.constraint_args(phrases, free_from, vocab, eot)
    if ct is None:
        raise ValueError("the list of phrases is empty")
    ids, off, n, ff = ct[1]
    B, stride = tok.shape
    node = np.zeros((steps + 1, B), np.int32)
    mask = np.zeros((steps + 1, B, (vocab + 31) // 32), np.uint32)
    ip, up = (lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))), (lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32)))
    _lib.check(_lib.lib().wm_op_constraint_states(ip(node), up(mask), ip(tok), ip(pl), ip(nn), B, stride, int(vocab), int(eot), int(ngram),
                                                  ip(ids), ip(off), n, ff, int(steps)))
    return node, mask


def _ip(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def _chk_i32(a, shape, name):
    if a is not None and (a.dtype != np.int32 or not a.flags.c_contiguous or a.shape != tuple(shape)):
        raise ValueError(f"{name} must be a C-contiguous int32 array of shape {tuple(shape)}")


def ts_states(tokens, prompt_len, n_ids, vocab: int, timestamp_begin: int, eos: int, max_initial=None, steps: int = 0, row_prompts: bool = False):
    """The timestamp rules' state machine alone (wm_op_ts_states): tokens / prompt_len / n_ids as repeat_sets; the real init
    launch (row_prompts: the ragged-rows form, else all rows share row 0's prompt), then one argmax launch per step that is handed the
    row's next id as its only candidate -> dict: states [steps + 1, B, 8] (TsState: n_gen, last_ts, pen_ts, t_last, text_lo, text_hi,
    ts_lo, ts_hi; entry 0 behind the init, entry s behind step s, a row's entries counting up to its own end), picks [steps, B], the final
    out_tokens [B, stride], n_tokens [B], pos [B], ctl [4], and with row_prompts key_lo [B], tok_rows / pos_rows [Lmax, B]."""
    tok = np.ascontiguousarray(tokens, np.int32)
    pl, nn = np.ascontiguousarray(prompt_len, np.int32).ravel(), np.ascontiguousarray(n_ids, np.int32).ravel()
    if tok.ndim != 2 or pl.size != tok.shape[0] or nn.size != tok.shape[0] or steps < 0:
        raise ValueError("tokens must be [B, stride], prompt_len and n_ids [B]")
    B, stride = tok.shape
    Lmax = max(1, int(pl.max()))
    r = dict(states=np.zeros((steps + 1, B, 8), np.int32), picks=np.zeros((steps, B), np.int32), out_tokens=np.zeros((B, stride), np.int32),
             n_tokens=np.zeros(B, np.int32), pos=np.zeros(B, np.int32), ctl=np.zeros(4, np.int32))
    if row_prompts:
        r.update(key_lo=np.zeros(B, np.int32), tok_rows=np.zeros((Lmax, B), np.int32), pos_rows=np.zeros((Lmax, B), np.int32))
    _lib.check(_lib.lib().wm_op_ts_states(_ip(r["states"]), _ip(r["picks"]), _ip(r["out_tokens"]), _ip(r["n_tokens"]), _ip(r["pos"]), _ip(r["ctl"]),
                                          _ip(r.get("key_lo")), _ip(r.get("tok_rows")), _ip(r.get("pos_rows")), _ip(tok), _ip(pl), _ip(nn), B, stride,
                                          int(vocab), int(timestamp_begin), int(eos), -1 if max_initial is None else int(max_initial), int(steps),
                                          int(bool(row_prompts))))
    return r


def init_tokens(bufs, B: int, prompt=None, table=None, lens=None, Lmax: int = 0, ts=None):
    """init_tokens_kernel (prompt: 1 .. 16 ids) or init_tokens_rows_kernel (table [B, stride] int32 with lens [B] and Lmax) alone
    (wm_op_init_tokens), in place on the caller's sentinel-filled int32 / float32 arrays `bufs`: out_tokens [B_held, out_stride],
    n_tokens, finished [B_held], ctl [4], and — each None or absent: the kernel gets a null pointer — tok_rows / pos_rows [rows_held, B],
    ts_state [B_held, 8] (then ts = (vocab, timestamp_begin, eos, max_initial or None)), logprobs [B_held, out_stride] with lp_sum
    [B_held], key_lo [B_held] (rows form)."""
    g = bufs.get
    out = g("out_tokens")
    if out is None or out.ndim != 2:
        raise ValueError("out_tokens must be [B_held, out_stride]")
    Bh, stride = out.shape
    _chk_i32(out, (Bh, stride), "out_tokens")
    for k in ("n_tokens", "finished", "key_lo"):
        _chk_i32(g(k), (Bh,), k)
    _chk_i32(g("ctl"), (4,), "ctl")
    _chk_i32(g("ts_state"), (Bh, 8), "ts_state")
    rows_held = 0
    if g("tok_rows") is not None:
        rows_held = g("tok_rows").shape[0]
        _chk_i32(g("tok_rows"), (rows_held, B), "tok_rows")
        _chk_i32(g("pos_rows"), (rows_held, B), "pos_rows")
    if g("logprobs") is not None:
        _chk_out(g("logprobs"), (Bh, stride))
        _chk_out(g("lp_sum"), (Bh,))
    if g("n_tokens") is None or g("finished") is None or g("ctl") is None:
        raise ValueError("n_tokens, finished and ctl are required")
    vocab, tb, eos, mi = ts if ts is not None else (0, 0, 0, None)
    if table is not None:
        p = np.ascontiguousarray(table, np.int32)
        ln = np.ascontiguousarray(lens, np.int32).ravel()
        if p.ndim != 2 or p.shape[0] != B or ln.size != B:
            raise ValueError("table must be [B, stride] and lens [B]")
        n_prompt, row_stride = 0, p.shape[1]
    else:
        p, ln = np.ascontiguousarray(prompt, np.int32).ravel(), None
        n_prompt, row_stride = p.size, 0
    _lib.check(_lib.lib().wm_op_init_tokens(_ip(out), _ip(g("n_tokens")), _ip(g("finished")), _ip(g("ctl")), _ip(g("tok_rows")), _ip(g("pos_rows")),
                                            _ip(g("ts_state")), _fp(g("logprobs")), _fp(g("lp_sum")), _ip(g("key_lo")), _ip(p), n_prompt, _ip(ln),
                                            row_stride, int(Lmax), rows_held, int(B), Bh, stride, int(vocab), int(tb), int(eos),
                                            -1 if mi is None else int(mi)))
    return bufs


def set_rows_step(ctl, pos, lens, Lmax: int, pos_delta: int, B: int):
    """set_rows_step_kernel alone (wm_op_set_rows_step), in place: ctl [4], pos [B_held] int32; lens [B]."""
    _chk_i32(ctl, (4,), "ctl")
    _chk_i32(pos, (pos.shape[0],), "pos")
    ln = np.ascontiguousarray(lens, np.int32).ravel()
    if ln.size != B:
        raise ValueError("lens must be [B]")
    _lib.check(_lib.lib().wm_op_set_rows_step(_ip(ctl), _ip(pos), _ip(ln), int(Lmax), int(pos_delta), int(B), pos.shape[0]))


def set_step(ctl, pos, tok, length: int, set_len: bool, pos_value: int, tok_value: int, B: int, B_held: int):
    """set_step_kernel alone (wm_op_set_step), in place: ctl [4]; pos, tok [B_held] int32 or None."""
    _chk_i32(ctl, (4,), "ctl")
    _chk_i32(pos, (B_held,), "pos")
    _chk_i32(tok, (B_held,), "tok")
    _lib.check(_lib.lib().wm_op_set_step(_ip(ctl), _ip(pos), _ip(tok), int(length), int(bool(set_len)), int(pos_value), int(tok_value), int(B), int(B_held)))


def pack_tokens(dst, out_tokens, n_tokens, rows: int, rows_cap: int, stride: int):
    """pack_tokens_kernel alone (wm_op_pack_tokens), in place on dst [rows_held, 1 + stride] int32: out_tokens [rows, out_stride],
    n_tokens [rows]."""
    _chk_i32(dst, (dst.shape[0], 1 + stride), "dst")
    o = np.ascontiguousarray(out_tokens, np.int32)
    n = np.ascontiguousarray(n_tokens, np.int32).ravel()
    if o.ndim != 2 or o.shape[0] < rows or n.size < rows:
        raise ValueError("out_tokens must be [rows, out_stride] and n_tokens [rows]")
    _lib.check(_lib.lib().wm_op_pack_tokens(_ip(dst), _ip(o), _ip(n), o.shape[1], int(rows), int(rows_cap), dst.shape[0], int(stride)))


def dec_embed(x, tok_emb, pos_emb, tok, pos):
    """dec_embed_kernel alone (wm_op_dec_embed), in place on x [B_held, d] float32: x[b] = tok_emb[tok[b]] + pos_emb[pos[b]], b < len(tok)."""
    te, pe = np.ascontiguousarray(tok_emb, np.float32), np.ascontiguousarray(pos_emb, np.float32)
    t, p = np.ascontiguousarray(tok, np.int32).ravel(), np.ascontiguousarray(pos, np.int32).ravel()
    if te.ndim != 2 or pe.ndim != 2 or te.shape[1] != pe.shape[1] or t.size != p.size or x.ndim != 2:
        raise ValueError("tok_emb [vocab, d], pos_emb [n_pos, d], tok and pos [B]")
    _chk_out(x, (x.shape[0], te.shape[1]))
    _lib.check(_lib.lib().wm_op_dec_embed(_fp(x), _fp(te), _fp(pe), _ip(t), _ip(p), t.size, x.shape[0], te.shape[1], te.shape[0], pe.shape[0]))


def rows_copy(out, rows, dst=None):
    """no_speech_capture_kernel (dst None: out[r] = rows[r]) or score_collect_kernel (out[dst[r]] = rows[r] where dst[r] >= 0) alone
    (wm_op_rows_copy), in place on out [out_rows, d] float32."""
    r = np.ascontiguousarray(rows, np.float32)
    if r.ndim != 2 or out.ndim != 2:
        raise ValueError("rows must be [n_rows, d] and out [out_rows, d]")
    _chk_out(out, (out.shape[0], r.shape[1]))
    d = None
    if dst is not None:
        d = np.ascontiguousarray(dst, np.int32).ravel()
        if d.size != r.shape[0]:
            raise ValueError("dst needs one entry per row")
    _lib.check(_lib.lib().wm_op_rows_copy(_fp(out), _fp(r), _ip(d), r.shape[0], out.shape[0], r.shape[1]))


def mel_transpose_pad(image, mel, dtype=DT_F32):
    """mel_transpose_pad_kernel alone (wm_op_mel_transpose_pad), in place on image [B_held, L + 2, Cp] float32 (rounded to dtype on the
    way in, widened on the way out): mel [B, C, L], Cp = C rounded up to 32."""
    m = np.ascontiguousarray(mel, np.float32)
    if m.ndim != 3 or image.ndim != 3:
        raise ValueError("mel must be [B, C, L] and image [B_held, L + 2, Cp]")
    B, Cc, L = m.shape
    _chk_out(image, (image.shape[0], L + 2, (Cc + 31) // 32 * 32))
    _lib.check(_lib.lib().wm_op_mel_transpose_pad(_fp(image), _fp(m), B, image.shape[0], Cc, L, dtype))
