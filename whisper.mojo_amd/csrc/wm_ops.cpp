// wm_ops.cpp — the wm_op_* test hooks of include/whisper_mi.h: each uploads host fp32 arrays, launches one or two kernels exactly as
// the runtime (whisper_mi.cpp) wires them, and copies the result back, for the float64 and known-answer tests.  Hooks that need the
// static helpers of a subsystem (alignment, the front end, resampling, chunking, scoring, long-form) live in that subsystem's source.
#include "wm_host.h"

#include <type_traits>

using namespace wm;

// ---- the hooks' transfers, each written once (wm_host.h) ------------------------------------------------------------------
int upload_bytes(DevBuf& b, const void* h, size_t n) {
    WMCHK(b.alloc(n));
    HIPCHK(hipMemcpy(b.p, h, n, hipMemcpyHostToDevice));
    return 0;
}
int upload_padded(DevBuf& b, const float* h, size_t n, size_t n_dev, int dt) {
    std::vector<float> padded(std::max(n, n_dev), 0.f);
    memcpy(padded.data(), h, n * 4);
    return upload(b, padded.data(), padded.size(), dt);
}
// widen n operand-dtype values on the host
static void widen_to_f32(const void* src, int dtype, size_t n, float* dst) {
    if (dtype == WM_F32) {
        memcpy(dst, src, n * 4);
        return;
    }
    const uint16_t* h = static_cast<const uint16_t*>(src);
    for (size_t i = 0; i < n; ++i) {
        if (dtype == WM_BF16) {
            const uint32_t u = (uint32_t)h[i] << 16;
            memcpy(&dst[i], &u, 4);
        } else {
            _Float16 hv;
            memcpy(&hv, &h[i], 2);
            dst[i] = (float)hv;
        }
    }
}
int download_f32(float* dst, const DevBuf& b, size_t n, int dt) {
    std::vector<unsigned char> h(n * dt_size(dt));
    HIPCHK(hipMemcpy(h.data(), b.p, h.size(), hipMemcpyDeviceToHost));
    widen_to_f32(h.data(), dt, n, dst);
    return 0;
}
int download_f32_rows(float* dst, const DevBuf& b, size_t rows, size_t cols, size_t ld, int dt) {
    const size_t es = dt_size(dt);
    std::vector<unsigned char> h(rows * cols * es);
    HIPCHK(hipMemcpy2D(h.data(), cols * es, b.p, ld * es, cols * es, rows, hipMemcpyDeviceToHost));
    widen_to_f32(h.data(), dt, rows * cols, dst);
    return 0;
}
int vocab_k_check(int K) {
    if (K != 128 && K != 384 && K != 512 && K != 768 && K != 1024) return fail(WM_E_ARG, "K must be 128, 384, 512, 768 or 1024 (the logits kernels' d_model)");
    return 0;
}
int upload_vocab_head(TmpDev& t, const float* x, const float* ln_g, const float* ln_b, const float* emb, int B, int N, int K, int dtype,
                      const float** dx, VocabHead* h) {
    DevBuf &x_d = t.add(), &g = t.add(), &be = t.add(), &w = t.add();
    WMCHK(upload(x_d, x, (size_t)B * K, WM_F32));
    WMCHK(upload(g, ln_g, K, WM_F32));
    WMCHK(upload(be, ln_b, K, WM_F32));
    WMCHK(upload(w, emb, (size_t)N * K, dtype));
    *dx = x_d.as<float>();
    *h = VocabHead{g.as<float>(), be.as<float>(), w.p, N, K};
    return 0;
}

// ---- op-level entry points (whisper_tensor.mojo) --------------------------------------------------------------------------

extern "C" int wm_op_matmul_nt(float* C, const float* A, const float* Bm, const float* bias, int M, int N, int K, int dtype) {
    if (!C || !A || !Bm || M <= 0 || N <= 0 || K <= 0) return fail(WM_E_ARG, "bad argument");
    if (K % 32) return fail(WM_E_ARG, "K must be a multiple of 32");
    if (dtype < 0 || dtype > 2) return fail(WM_E_ARG, "bad dtype");
    TmpDev t;
    hipStream_t st = nullptr;
    if (N % 128 == 0) {  // dense path: the encoder GEMM kernel
        DevBuf &a = t.add(), &w = t.add(), &c = t.add(), &b = t.add();
        WMCHK(upload_padded(a, A, (size_t)M * K, panel_rows(M) * K, dtype));
        WMCHK(upload(w, Bm, (size_t)N * K, dtype));
        WMCHK(c.alloc((size_t)M * N * 4));
        if (bias) WMCHK(upload(b, bias, N, WM_F32));
        GemmParams p{};
        p.A = a.p;
        p.W = w.p;
        p.C = c.p;
        p.M = M;
        p.N = N;
        p.K = K;
        p.lda = K;
        p.ldw = K;
        p.ldc = N;
        p.bias = bias ? b.as<float>() : nullptr;
        WMCHK(gemm_dispatch(dtype, WM_F32, p, 1, st));
        HIPCHK(hipMemcpy(C, c.p, (size_t)M * N * 4, hipMemcpyDeviceToHost));
    } else {  // skinny path: the decode-step linear kernel
        const int Np = (N + 15) / 16 * 16;
        // the kernel splits K over NW <= 16 waves, <= 4 k-steps of 32 each: zero-pad K to the next such size
        auto splittable = [](int k) {
            const int ks = k / 32;
            for (int c = 16; c >= 1; --c)
                if (ks % c == 0 && ks / c <= 4) return true;
            return false;
        };
        int Kp = (K + 127) / 128 * 128;
        while (Kp <= 2048 && !splittable(Kp)) Kp += 128;  // (bounded: no K above 2048 splits, and an unbounded search overflowed)
        if (Kp > 2048) return fail(WM_E_ARG, "K too large for the skinny path (<= 2048)");
        std::vector<float> Apad((size_t)M * Kp, 0.f), Bpad((size_t)N * Kp, 0.f);
        for (int i = 0; i < M; ++i) memcpy(&Apad[(size_t)i * Kp], A + (size_t)i * K, (size_t)K * 4);
        for (int i = 0; i < N; ++i) memcpy(&Bpad[(size_t)i * Kp], Bm + (size_t)i * K, (size_t)K * 4);
        K = Kp;
        DevBuf &a = t.add(), &w = t.add(), &c = t.add(), &b = t.add();
        WMCHK(upload(a, Apad.data(), Apad.size(), WM_F32));
        WMCHK(upload(w, Bpad.data(), Bpad.size(), dtype));
        WMCHK(c.alloc((size_t)M * Np * 4));
        if (bias) WMCHK(upload(b, bias, N, WM_F32));
        DecLinearParams p{};
        p.x = a.as<float>();
        p.ldx = K;
        p.W = w.p;
        p.N = N;
        p.K = K;
        p.B = M;
        p.bias = bias ? b.as<float>() : nullptr;
        p.out = c.as<float>();
        p.ldo = Np;
        WMCHK(dec_linear_dispatch(dtype, p, st));
        WMCHK(download_f32_rows(C, c, M, N, Np, WM_F32));
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// C = layer_norm(A, ln_g, ln_b) · Bᵀ (+ bias): the LN -> projection pair of ResidualAttentionBlock.forward (layers.mojo:449-455,
// 489-497) on the encoder's kernels.  require_fused != 0 demands the ONE-kernel form (LayerNorm applied while the row-panel GEMM
// loads its fp32 A rows): a shape that kernel does not take is refused by the launcher — WM_E_ARG, nothing launched, C untouched.
extern "C" int wm_op_ln_matmul_nt(float* C, const float* A, const float* ln_g, const float* ln_b, const float* Bm, const float* bias,
                                  int M, int N, int K, int dtype, int require_fused) {
    if (!C || !A || !ln_g || !ln_b || !Bm || M <= 0 || N <= 0 || K <= 0) return fail(WM_E_ARG, "bad argument");
    if (dtype < 0 || dtype > 2) return fail(WM_E_ARG, "bad dtype");
    if (K % 128 || K > 1024) return fail(WM_E_ARG, "K must be a multiple of 128 and <= 1024 (layer_norm rows)");
    TmpDev t;
    hipStream_t st = nullptr;
    const size_t Mp = panel_rows(M);
    DevBuf &x = t.add(), &xn = t.add(), &w = t.add(), &c = t.add(), &b = t.add(), &g = t.add(), &be = t.add();
    WMCHK(upload_padded(x, A, (size_t)M * K, Mp * K, WM_F32));
    WMCHK(xn.alloc(Mp * K * dt_size(dtype), true));
    WMCHK(upload(w, Bm, (size_t)N * K, dtype));
    WMCHK(c.alloc((size_t)M * N * 4));
    WMCHK(upload(g, ln_g, K, WM_F32));
    WMCHK(upload(be, ln_b, K, WM_F32));
    if (bias) WMCHK(upload(b, bias, N, WM_F32));
    GemmParams p{};
    p.A = xn.p;
    p.W = w.p;
    p.C = c.p;
    p.M = M;
    p.N = N;
    p.K = K;
    p.lda = K;
    p.ldw = K;
    p.ldc = N;
    p.bias = bias ? b.as<float>() : nullptr;
    if (require_fused) {  // handed to the launcher as asked: it either fuses or refuses
        p.A = x.p;
        p.ln_g = g.as<float>();
        p.ln_b = be.as<float>();
        WMCHK(gemm_dispatch(dtype, WM_F32, p, 1, st));
    } else {
        WMCHK(ln_then_gemm(dtype, WM_F32, p, x.as<float>(), g.as<float>(), be.as<float>(), st));
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(C, c.p, (size_t)M * N * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int wm_op_layer_norm(float* out, const float* inp, const float* gamma, const float* beta, int rows, int cols, float eps) {
    if (!out || !inp || !gamma || !beta || rows <= 0 || cols <= 0) return fail(WM_E_ARG, "bad argument");
    if (cols % 128 || cols > 1024) return fail(WM_E_ARG, "cols must be a multiple of 128 and <= 1024");
    TmpDev t;
    DevBuf &x = t.add(), &g = t.add(), &b = t.add(), &o = t.add();
    WMCHK(upload(x, inp, (size_t)rows * cols, WM_F32));
    WMCHK(upload(g, gamma, cols, WM_F32));
    WMCHK(upload(b, beta, cols, WM_F32));
    WMCHK(o.alloc((size_t)rows * cols * 4));
    launch_layernorm_rows<float>(x.as<float>(), g.as<float>(), b.as<float>(), nullptr, o.as<float>(), rows, cols, eps, nullptr);
    HIPCHK(hipMemcpy(out, o.p, (size_t)rows * cols * 4, hipMemcpyDeviceToHost));
    return 0;
}

// launch_layernorm_rows<T> with the operand-dtype store (out_t, returned widened), the fp32 store (out_f), or both — the launches the
// base / small encoder makes before every projection.  out_t / out_f hold rows + 1 rows, in and out: the device buffers start from the
// caller's values, so the guard row (and anything else the kernel did not write) comes back as it went in.  Known-answer tests.
extern "C" int wm_op_layer_norm_t(float* out_t, float* out_f, const float* inp, const float* gamma, const float* beta, int rows, int cols,
                                  float eps, int dtype) {
    if ((!out_t && !out_f) || !inp || !gamma || !beta || rows <= 0 || cols <= 0) return fail(WM_E_ARG, "bad argument");
    if (dtype < 0 || dtype > 2) return fail(WM_E_ARG, "bad dtype");
    if (cols % 128 || cols > 1024) return fail(WM_E_ARG, "cols must be a multiple of 128 and <= 1024");
    const size_t n = (size_t)rows * cols, ng = n + cols;
    TmpDev t;
    DevBuf &x = t.add(), &g = t.add(), &b = t.add(), &ot = t.add(), &of = t.add();
    WMCHK(upload(x, inp, n, WM_F32));
    WMCHK(upload(g, gamma, cols, WM_F32));
    WMCHK(upload(b, beta, cols, WM_F32));
    if (out_t) WMCHK(upload(ot, out_t, ng, dtype));
    if (out_f) WMCHK(upload(of, out_f, ng, WM_F32));
    DISPATCH_DT(dtype, TT, launch_layernorm_rows<TT>(x.as<float>(), g.as<float>(), b.as<float>(), out_t ? ot.p : nullptr,
                                                     out_f ? of.as<float>() : nullptr, rows, cols, eps, nullptr));
    HIPCHK(hipGetLastError());
    if (out_t) WMCHK(download_f32(out_t, ot, ng, dtype));
    if (out_f) HIPCHK(hipMemcpy(out_f, of.p, ng * 4, hipMemcpyDeviceToHost));
    return 0;
}

// One gemm_dispatch call with everything GemmParams offers (include/whisper_mi.h), behind wm_op_gemm_nt_epi (ring == false: the two
// tiled kernels) and wm_op_gemm_nt_ring (ring == true: the row-panel and full-row kernels).
// Device sizes, tiled kernels: both read whole 128-row panels of A whatever M is, so A is allocated zero-filled up to the last panel
// row; bias, pos, residual and C are touched at valid rows only (gemm_epilogue's valid[]), and the checks below hold every offset the
// epilogue can form inside the caller's lengths, which are also the device lengths.
// Device sizes, ring kernels (read off kernels_encoder.hip): both clamp a row index >= M to M - 1 before they form any address —
// gemm_nt_rowpanel_kernel `row = row < p.M ? row : p.M - 1` for its A fragments (16-bit, or the fp32 rows of the LNA form), the
// full-row kernel `ar = ar < p.M ? ar : p.M - 1` for its A DMA and `mrow[i]` for residual, pos and the C row pointer — so A is read at
// bz·strideA + row·lda + [0, K) with row < M only, residual at bz·strideR + row·ldr + [0, N), pos at row·N + [0, N), W at all N rows
// of K, bias / ln_g / ln_b / lno_g / lno_b whole.  Stores are masked by row < M (`m >= p.M`, `mbase + row < p.M`, `valid`, `m < p.M`),
// C at (group)·group_stride + bz·strideC + m·ldc + [0, row width), lno_out at bz·strideC + m·ldc + [0, N) in the operand type.  The
// caller's lengths therefore cover both kernels; A is still zero-filled up to the end of the last 128-row panel, as upload_padded
// callers do everywhere.  The full-row kernel forms its A offsets inside a batch in 32 bits: (M - 1)·lda + K must stay below 2^31
// elements.  The 16-bit stores of both kernels are 16 bytes wide: ldc, strideC and group_stride are then multiples of 8.
static int op_gemm_nt(bool ring, float* C, size_t c_len, const float* A, size_t a_len, const float* W, const float* bias, const float* pos,
                      const float* residual, size_t r_len, int M, int N, int K, int batch, long long lda, long long strideA, long long ldc,
                      long long strideC, long long ldr, long long strideR, int residual_in_place, int act, int gelu_mode, int group_n,
                      long long group_stride, int dtype, int out_dtype, const float* ln_g, const float* ln_b, const float* lno_g,
                      const float* lno_b, float* lno_out, size_t lno_len, int* kernel_ran) {
    if (!C || !A || !W || !kernel_ran || M <= 0 || N <= 0 || K <= 0 || batch <= 0) return fail(WM_E_ARG, "bad argument");
    if (M > (1 << 20) || N > (1 << 16) || K > (1 << 16) || batch > 1024) return fail(WM_E_ARG, "problem too large for the op hook");
    if (dtype < 0 || dtype > 2) return fail(WM_E_ARG, "bad dtype");
    if (out_dtype != WM_F32 && out_dtype != dtype) return fail(WM_E_ARG, "out_dtype must be WM_F32 or dtype");
    if (N % 128 || K % 32) return fail(WM_E_ARG, "N must be a multiple of 128 and K of 32");
    if ((act != 0 && act != 1) || (gelu_mode != 0 && gelu_mode != 1)) return fail(WM_E_ARG, "bad act / gelu_mode");
    const long long LIM = 1ll << 40;  // keeps every product below int64
    auto ld_ok = [&](long long v, int unit, bool zero_ok) { return (v > 0 || (zero_ok && v == 0)) && v < LIM && v % unit == 0; };
    // 16-byte operand loads: 8 sixteen-bit or 4 fp32 elements (8 serves both); 16-byte fp32 / 8-byte 16-bit stores and addend loads: 4
    if (!ld_ok(lda, 8, false) || !ld_ok(strideA, 8, true) || !ld_ok(ldc, 4, false) || !ld_ok(strideC, 4, true))
        return fail(WM_E_ARG, "lda / strideA must be multiples of 8, ldc / strideC of 4");
    if (batch > 1 && (strideA == 0 || strideC == 0)) return fail(WM_E_ARG, "batch > 1 needs strideA and strideC");
    if (group_n < 0 || group_n % 64 || (group_n > 0 && (N % group_n || !ld_ok(group_stride, 4, false))))
        return fail(WM_E_ARG, "group_n must be a multiple of 64 that divides N, with a group_stride that is a multiple of 4");
    const int n_grp = group_n > 0 ? N / group_n : 1, row_w = group_n > 0 ? group_n : N;
    if (ldc < row_w) return fail(WM_E_ARG, "ldc below the row width");
    if (residual_in_place) {
        if (out_dtype != WM_F32) return fail(WM_E_ARG, "residual_in_place needs fp32 output");
        if (residual || group_n > 0) return fail(WM_E_ARG, "residual_in_place takes no separate residual and no column groups");
        ldr = ldc;
        strideR = strideC;
    } else if (residual) {
        if (!ld_ok(ldr, 4, false) || !ld_ok(strideR, 4, true) || ldr < N || (batch > 1 && strideR == 0))
            return fail(WM_E_ARG, "ldr must be a multiple of 4 and >= N, strideR a multiple of 4");
    }
    const size_t Mp = panel_rows(M);
    const size_t a_need = (size_t)(batch - 1) * strideA + (size_t)(M - 1) * lda + K;
    const size_t a_dev = (size_t)(batch - 1) * strideA + (Mp - 1) * (size_t)lda + K;
    const size_t c_need = (size_t)(batch - 1) * strideC + (size_t)(n_grp - 1) * (group_n > 0 ? group_stride : 0) + (size_t)(M - 1) * ldc + row_w;
    const size_t r_need = (size_t)(batch - 1) * strideR + (size_t)(M - 1) * ldr + N;
    if (a_len < a_need || c_len < c_need || (residual && r_len < r_need)) return fail(WM_E_ARG, "a size overflows the caller's arrays");
    if (a_len > ((size_t)1 << 31) || c_len > ((size_t)1 << 31) || r_len > ((size_t)1 << 31)) return fail(WM_E_ARG, "array too large for the op hook");
    if ((ln_g != nullptr) != (ln_b != nullptr)) return fail(WM_E_ARG, "ln_g and ln_b go together");
    const bool lno = lno_g || lno_b || lno_out;
    if (lno && (!lno_g || !lno_b || !lno_out)) return fail(WM_E_ARG, "lno_g, lno_b and lno_out go together");
    if (ring) {
        if ((size_t)(M - 1) * lda + K >= ((size_t)1 << 31)) return fail(WM_E_ARG, "rows of one batch reach past 2^31 elements");
        const bool wide = out_dtype != WM_F32 || lno;  // 16-byte stores of eight 16-bit elements
        if (wide && (ldc % 8 || strideC % 8 || (group_n > 0 && group_stride % 8)))
            return fail(WM_E_ARG, "16-bit rows need ldc / strideC / group_stride that are multiples of 8");
        if (lno && (lno_len < c_need || lno_len > ((size_t)1 << 31))) return fail(WM_E_ARG, "lno_len does not hold the rows");
    }
    TmpDev t;
    DevBuf &a = t.add(), &w = t.add(), &c = t.add(), &b = t.add(), &ps = t.add(), &r = t.add(), &g1 = t.add(), &b1 = t.add(), &g2 = t.add(),
           &b2 = t.add(), &lo = t.add();
    GemmParams p{};
    p.M = M;
    p.N = N;
    p.K = K;
    p.lda = (long)lda;
    p.ldw = K;
    p.ldc = (long)ldc;
    p.strideA = (long)strideA;
    p.strideC = (long)strideC;
    p.ldr = (long)ldr;
    p.strideR = (long)strideR;
    p.act = act;
    p.gelu_mode = gelu_mode;
    p.group_n = group_n;
    p.group_stride = group_n > 0 ? (long)group_stride : 0;
    // addend pointers decide the dispatch (the row-panel kernel takes none): non-null placeholders until the uploads below
    p.bias = bias;
    p.pos = pos;
    p.residual = residual_in_place ? C : residual;
    p.ln_g = ln_g;  // handed to the launcher as asked: a shape that cannot fuse is refused
    p.ln_b = ln_b;
    p.lno_g = lno_g;
    p.lno_b = lno_b;
    p.lno_out = lno_out;
    const char* why = "";
    *kernel_ran = gemm_nt_kernel_for((int)dt_size(dtype), (int)dt_size(out_dtype), p, batch, &why);
    if (*kernel_ran == wm::GEMM_NT_REFUSED) return fail(WM_E_ARG, why);
    const bool is_ring = *kernel_ran == wm::GEMM_NT_ROWPANEL || *kernel_ran == wm::GEMM_NT_FULLROW;
    // the tiled hook's device sizes are worked out for the two tiled kernels only; the ring kernels have a hook of their own
    if (!ring && is_ring)
        return fail(WM_E_ARG, "this shape dispatches to the row-panel / full-row kernel (wm_op_matmul_nt, wm_op_ln_matmul_nt, wm_op_mlp_block)");
    if (ring && !is_ring) return fail(WM_E_ARG, "this shape dispatches to a tiled kernel (wm_op_gemm_nt_epi)");
    // A: the caller's part, then zeros up to the end of the last 128-row panel (fp32 rows where the row-panel kernel normalises them)
    WMCHK(upload_padded(a, A, a_need, a_dev, ln_g ? WM_F32 : dtype));
    WMCHK(upload(w, W, (size_t)N * K, dtype));
    WMCHK(upload(c, C, c_len, out_dtype));
    if (bias) WMCHK(upload(b, bias, N, WM_F32));
    if (pos) WMCHK(upload(ps, pos, (size_t)M * N, WM_F32));
    if (residual && !residual_in_place) WMCHK(upload(r, residual, r_len, WM_F32));
    if (ln_g) {
        WMCHK(upload(g1, ln_g, K, WM_F32));
        WMCHK(upload(b1, ln_b, K, WM_F32));
    }
    if (lno) {  // the 16-bit rows start from the caller's values: what the kernel leaves alone comes back as it went in
        WMCHK(upload(g2, lno_g, N, WM_F32));
        WMCHK(upload(b2, lno_b, N, WM_F32));
        WMCHK(upload(lo, lno_out, lno_len, dtype));
    }
    p.A = a.p;
    p.W = w.p;
    p.C = c.p;
    p.bias = bias ? b.as<float>() : nullptr;
    p.pos = pos ? ps.as<float>() : nullptr;
    p.residual = residual_in_place ? c.as<float>() : residual ? r.as<float>() : nullptr;
    p.ln_g = ln_g ? g1.as<float>() : nullptr;
    p.ln_b = ln_g ? b1.as<float>() : nullptr;
    p.lno_g = lno ? g2.as<float>() : nullptr;
    p.lno_b = lno ? b2.as<float>() : nullptr;
    p.lno_out = lno ? lo.p : nullptr;
    WMCHK(gemm_dispatch(dtype, out_dtype, p, batch, nullptr));
    HIPCHK(hipGetLastError());
    if (lno) WMCHK(download_f32(lno_out, lo, lno_len, dtype));
    return download_f32(C, c, c_len, out_dtype);
}

extern "C" int wm_op_gemm_nt_epi(float* C, size_t c_len, const float* A, size_t a_len, const float* W, const float* bias, const float* pos,
                                 const float* residual, size_t r_len, int M, int N, int K, int batch, long long lda, long long strideA,
                                 long long ldc, long long strideC, long long ldr, long long strideR, int residual_in_place, int act,
                                 int gelu_mode, int group_n, long long group_stride, int dtype, int out_dtype, int* kernel_ran) {
    return op_gemm_nt(false, C, c_len, A, a_len, W, bias, pos, residual, r_len, M, N, K, batch, lda, strideA, ldc, strideC, ldr, strideR,
                      residual_in_place, act, gelu_mode, group_n, group_stride, dtype, out_dtype, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                      kernel_ran);
}

// wm_op_gemm_nt_epi's twin for the shapes the launcher gives to gemm_nt_rowpanel_kernel and gemm_nt_fullrow_kernel, with the two
// fused LayerNorms those kernels carry (op_gemm_nt's comment has the device-size argument).
extern "C" int wm_op_gemm_nt_ring(float* C, size_t c_len, const float* A, size_t a_len, const float* W, const float* bias, const float* pos,
                                  const float* residual, size_t r_len, int M, int N, int K, int batch, long long lda, long long strideA,
                                  long long ldc, long long strideC, long long ldr, long long strideR, int residual_in_place, int act,
                                  int gelu_mode, int group_n, long long group_stride, int dtype, int out_dtype, const float* ln_g,
                                  const float* ln_b, const float* lno_g, const float* lno_b, float* lno_out, size_t lno_len, int* kernel_ran) {
    return op_gemm_nt(true, C, c_len, A, a_len, W, bias, pos, residual, r_len, M, N, K, batch, lda, strideA, ldc, strideC, ldr, strideR,
                      residual_in_place, act, gelu_mode, group_n, group_stride, dtype, out_dtype, ln_g, ln_b, lno_g, lno_b, lno_out, lno_len,
                      kernel_ran);
}

extern "C" int wm_op_mlp_block(float* x, const float* ln_g, const float* ln_b, const float* fc1_w, const float* fc1_b, const float* fc2_w,
                               const float* fc2_b, const float* next_g, const float* next_b, float* xn_out, int M, int d, int ffn,
                               int dtype, int gelu_mode) {
    if (!x || !ln_g || !ln_b || !fc1_w || !fc1_b || !fc2_w || !fc2_b || M <= 0) return fail(WM_E_ARG, "bad argument");
    if (d <= 0 || d % 128 || d > 1024 || ffn <= 0 || ffn % 128) return fail(WM_E_ARG, "d and ffn must be multiples of 128 (d <= 1024)");
    if (dtype < 0 || dtype > 2 || (gelu_mode != 0 && gelu_mode != 1)) return fail(WM_E_ARG, "bad dtype / gelu_mode");
    const bool want_next = next_g && next_b && xn_out;
    if (!want_next && (next_g || next_b || xn_out)) return fail(WM_E_ARG, "next_g, next_b and xn_out go together");
    TmpDev t;
    hipStream_t st = nullptr;
    const size_t Mp = panel_rows(M), ts = dt_size(dtype);  // the tile kernels read whole 128-row panels
    DevBuf &dx = t.add(), &xn = t.add(), &hid = t.add(), &g1 = t.add(), &b1 = t.add(), &w1 = t.add(), &bb1 = t.add(), &w2 = t.add(),
           &bb2 = t.add(), &g2 = t.add(), &b2 = t.add();
    WMCHK(upload_padded(dx, x, (size_t)M * d, Mp * d, WM_F32));
    WMCHK(xn.alloc(Mp * d * ts, true));
    WMCHK(hid.alloc(Mp * ffn * ts, true));
    WMCHK(upload(g1, ln_g, d, WM_F32));
    WMCHK(upload(b1, ln_b, d, WM_F32));
    WMCHK(upload(w1, fc1_w, (size_t)ffn * d, dtype));
    WMCHK(upload(bb1, fc1_b, ffn, WM_F32));
    WMCHK(upload(w2, fc2_w, (size_t)d * ffn, dtype));
    WMCHK(upload(bb2, fc2_b, d, WM_F32));
    if (want_next) {
        WMCHK(upload(g2, next_g, d, WM_F32));
        WMCHK(upload(b2, next_b, d, WM_F32));
    }
    GemmParams f1{};
    f1.A = xn.p;
    f1.W = w1.p;
    f1.C = hid.p;
    f1.M = M;
    f1.N = ffn;
    f1.K = d;
    f1.lda = d;
    f1.ldw = d;
    f1.ldc = ffn;
    f1.bias = bb1.as<float>();
    f1.act = 1;
    f1.gelu_mode = gelu_mode;
    WMCHK(ln_then_gemm(dtype, dtype, f1, dx.as<float>(), g1.as<float>(), b1.as<float>(), st));
    GemmParams f2{};
    f2.A = hid.p;
    f2.W = w2.p;
    f2.C = dx.p;
    f2.M = M;
    f2.N = d;
    f2.K = ffn;
    f2.lda = ffn;
    f2.ldw = ffn;
    f2.ldc = d;
    f2.bias = bb2.as<float>();
    f2.residual = dx.as<float>();
    f2.ldr = d;
    bool fused_next = false;
    if (want_next && gemm_nt_fuses_layernorm_out(dtype == WM_F32 ? 4 : 2, f2)) {
        f2.lno_g = g2.as<float>();
        f2.lno_b = b2.as<float>();
        f2.lno_out = xn.p;
        fused_next = true;
    }
    WMCHK(gemm_dispatch(dtype, WM_F32, f2, 1, st));
    if (want_next && !fused_next)
        DISPATCH_DT(dtype, TT, launch_layernorm_rows<TT>(dx.as<float>(), g2.as<float>(), b2.as<float>(), xn.p, nullptr, M, d, 1e-5f, st));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(x, dx.p, (size_t)M * d * 4, hipMemcpyDeviceToHost));
    if (want_next) WMCHK(download_f32(xn_out, xn, (size_t)M * d, dtype));  // the operand rows as the next GEMM reads them, widened on the host
    return 0;
}

extern "C" int wm_op_attention_batch(float* out, const float* q, const float* k, const float* v, int B, int n_ctx, int n_heads, int dtype) {
    if (!out || !q || !k || !v || B <= 0 || n_ctx <= 0 || n_heads <= 0 || n_heads > 64) return fail(WM_E_ARG, "bad argument");
    if (dtype < 0 || dtype > 2) return fail(WM_E_ARG, "bad dtype");
    const size_t d = (size_t)n_heads * 64, rows = (size_t)B * n_ctx, n = rows * d;
    std::vector<float> packed(3 * n);  // the fused projection layout the kernel reads: row = [q | k | v], utterances back to back
    for (size_t t = 0; t < rows; ++t) {
        memcpy(&packed[t * 3 * d], q + t * d, d * 4);
        memcpy(&packed[t * 3 * d + d], k + t * d, d * 4);
        memcpy(&packed[t * 3 * d + 2 * d], v + t * d, d * 4);
    }
    TmpDev t;
    DevBuf &qkv = t.add(), &o = t.add();
    WMCHK(upload(qkv, packed.data(), packed.size(), dtype));
    WMCHK(o.alloc(n * dt_size(dtype), true));
    DISPATCH_DT(dtype, TT, launch_flash_attn_enc<TT>(qkv.p, o.p, B, n_heads, n_ctx, 0.125f, nullptr));
    HIPCHK(hipGetLastError());
    return download_f32(out, o, n, dtype);
}
extern "C" int wm_op_attention(float* out, const float* q, const float* k, const float* v, int n_ctx, int n_heads, int dtype) {
    return wm_op_attention_batch(out, q, k, v, 1, n_ctx, n_heads, dtype);
}

static int op_attention_cached(float* out, const float* q, const float* k, const float* v, int B, int t, int n_heads, int kv_dtype,
                               int n_chunks, int out_dtype, int q_B, int len, int nq, const int32_t* key_lo, bool with_lo,
                               const int32_t* utt_of = nullptr, int n_map_utt = 0);
extern "C" int wm_op_attention_cached(float* out, const float* q, const float* k, const float* v, int B, int t, int n_heads, int kv_dtype,
                                      int n_chunks, int out_dtype, int q_B, int len, int nq) {
    return op_attention_cached(out, q, k, v, B, t, n_heads, kv_dtype, n_chunks, out_dtype, q_B, len, nq, nullptr, false);
}
extern "C" int wm_op_attention_cached_lo(float* out, const float* q, const float* k, const float* v, int B, int t, int n_heads, int kv_dtype,
                                         int n_chunks, int out_dtype, int q_B, int len, int nq, const int32_t* key_lo) {
    return op_attention_cached(out, q, k, v, B, t, n_heads, kv_dtype, n_chunks, out_dtype, q_B, len, nq, key_lo, true);
}
// The chunked cross-attention forms with K/V by row map: k, v hold n_utt clips of t rows, the row in batch slot b (of q_B
// slots, or of B when q_B == 0) reads clip utt_of[b].
extern "C" int wm_op_attention_cached_map(float* out, const float* q, const float* k, const float* v, int B, int t, int n_heads, int kv_dtype,
                                          int n_chunks, int out_dtype, int q_B, int len, int nq, const int32_t* utt_of, int n_utt) {
    if (!utt_of || n_utt < 1 || n_chunks < 2) return fail(WM_E_ARG, "the map belongs to the chunked forms (n_chunks >= 2) and needs n_utt >= 1 clips");
    return op_attention_cached(out, q, k, v, B, t, n_heads, kv_dtype, n_chunks, out_dtype, q_B, len, nq, nullptr, false, utt_of, n_utt);
}
static int op_attention_cached(float* out, const float* q, const float* k, const float* v, int B, int t, int n_heads, int kv_dtype,
                               int n_chunks, int out_dtype, int q_B, int len, int nq, const int32_t* key_lo, bool with_lo,
                               const int32_t* utt_of, int n_map_utt) {
    if (with_lo && (!key_lo || n_chunks != 1 || nq != 0)) return fail(WM_E_ARG, "key_lo belongs to the single-workgroup forms (n_chunks = 1, nq = 0)");
    if (!out || !q || !k || !v || B <= 0 || t <= 0 || n_heads <= 0 || n_heads > 16) return fail(WM_E_ARG, "bad argument");
    if (kv_dtype < 0 || kv_dtype > 2 || out_dtype < 0 || out_dtype > 2) return fail(WM_E_ARG, "bad dtype");
    if (n_chunks < 1 || (n_chunks > 1 && (n_chunks < (t + 511) / 512 || n_chunks > (t + 31) / 32)))
        return fail(WM_E_ARG, "n_chunks must be 1, or between ceil(t/512) and ceil(t/32)");
    if (n_chunks == 1 && t > 512) return fail(WM_E_ARG, "the single-workgroup form serves up to 512 keys (the text context)");
    if (n_chunks > 64) return fail(WM_E_ARG, "the merge takes up to 64 chunks");
    if (q_B < 0 || (q_B > 0 && B % q_B)) return fail(WM_E_ARG, "prefill rows are position-major: B must be P * q_B");
    if (nq != 0 && (nq != 4 || n_chunks == 1 || q_B == 0 || B != 4 * q_B))
        return fail(WM_E_ARG, "nq must be 0, or 4 with the chunked form and B = 4 * q_B rows");
    const int P = q_B > 0 ? B / q_B : 1, n_slots = q_B > 0 ? q_B : B;
    const int n_utt = utt_of ? n_map_utt : n_slots;  // k, v hold n_utt utterances of t rows
    if (n_chunks > 1 && len >= 0) return fail(WM_E_ARG, "len belongs to the single-workgroup form (the chunked form sweeps all t rows)");
    if (n_chunks == 1 && len < 0 && P > 1) return fail(WM_E_ARG, "the causal prefill form needs len >= 0");
    if (n_chunks == 1 && len >= 0 && len + P > t) return fail(WM_E_ARG, "the cache must hold len + P rows");
    const size_t d = (size_t)n_heads * 64, n = (size_t)B * d;
    TmpDev tmp;
    DevBuf &dq = tmp.add(), &dk = tmp.add(), &dv = tmp.add(), &po = tmp.add(), &pml = tmp.add(), &o = tmp.add(), &ctl = tmp.add(), &dlo = tmp.add();
    DevBuf& dmap = tmp.add();
    if (utt_of) {
        for (int b = 0; b < n_slots; ++b)
            if (utt_of[b] < 0 || utt_of[b] >= n_utt) return fail(WM_E_ARG, "utt_of[%d] = %d outside [0, %d)", b, utt_of[b], n_utt);
        WMCHK(upload_bytes(dmap, utt_of, (size_t)n_slots * 4));
    }
    if (with_lo) {
        for (int u = 0; u < n_utt; ++u)
            if (key_lo[u] < 0 || key_lo[u] > t) return fail(WM_E_ARG, "key_lo[%d] = %d outside [0, %d]", u, key_lo[u], t);
        WMCHK(upload_bytes(dlo, key_lo, (size_t)n_utt * 4));
    }
    WMCHK(upload(dq, q, n, WM_F32));
    WMCHK(upload(dk, k, (size_t)n_utt * t * d, kv_dtype));
    WMCHK(upload(dv, v, (size_t)n_utt * t * d, kv_dtype));
    WMCHK(o.alloc(n * dt_size(out_dtype), true));
    AttnDecParams a{};
    a.q = dq.as<float>();
    a.K = dk.p;
    a.V = dv.p;
    a.batch_stride = (long)((size_t)t * d);
    a.scale = 0.125f;
    a.H = n_heads;
    a.d = (int)d;
    a.B = B;
    a.q_B = q_B;
    a.nq = nq;
    if (n_chunks > 1) {
        WMCHK(po.alloc((size_t)B * n_chunks * d * 4, true));
        WMCHK(pml.alloc((size_t)B * n_chunks * n_heads * 2 * 4, true));
        a.n_keys = t;
        a.nsplit = n_chunks;
        a.part_o = po.as<float>();
        a.part_ml = pml.as<float>();
        WMCHK(attn_decode_dispatch(kv_dtype, a, nullptr, nullptr, utt_of ? dmap.as<int>() : nullptr));
        launch_attn_combine(po.as<float>(), pml.as<float>(), o.p, out_dtype, B, n_chunks, n_heads, (int)d, nullptr);
    } else {
        StepCtl h{};
        // the kernel sweeps len + 1 rows (position p of a prefill: len + 1 + p): the cache as it stands after this step's row was appended
        h.len = len >= 0 ? len : t - 1;
        WMCHK(upload_bytes(ctl, &h, sizeof h));
        a.n_keys = -1;
        a.ctl = ctl.as<StepCtl>();
        a.nsplit = 1;
        a.direct_out = o.as<float>();
        a.out_dtype = out_dtype;
        WMCHK(attn_decode_dispatch(kv_dtype, a, nullptr, with_lo ? dlo.as<int>() : nullptr));
    }
    HIPCHK(hipGetLastError());
    return download_f32(out, o, n, out_dtype);
}

// One launch_dec_linear as decode_core wires it: LN1 -> QKV with the cache append, the XT out-projections with the residual in place,
// LNx -> cross q with the alignment-head capture, LN2 -> fc1 + GELU stored in operand dtype, fc2.
// cap_map non-null: the capture by row map, cap is [cap_dst][cap_nsel][64] and len / cap_step0 / cap_steps are not used
static int op_dec_linear(float* out, const float* x, const float* W, const float* bias, const float* ln_g, const float* ln_b,
                         const float* residual, int B, int N, int K, int dtype, int x_is_t, int out_is_t, int act, int gelu_mode,
                         float* kcache, float* vcache, int n_utt, int cap_rows, int kv_dtype, int kv_B, int len, float* cap,
                         const int8_t* cap_sel, int cap_step0, int cap_steps, int cap_nsel, const int32_t* cap_map = nullptr, int cap_dst = 0,
                         bool k_long = false) {
    if (!out || !x || !W || B <= 0 || N <= 0 || K <= 0) return fail(WM_E_ARG, "bad argument");
    if (dtype < 0 || dtype > 2 || (gelu_mode != 0 && gelu_mode != 1)) return fail(WM_E_ARG, "bad dtype / gelu_mode");
    if (k_long) {  // wm_op_dec_linear_long: the K-long form alone (16 waves walking groups of k-steps), which has no LayerNorm prologue
        if (!dec_linear_long_supports_k(K)) return fail(WM_E_ARG, "K must be 3072 or 4096 (the K-long form of the skinny linear)");
        if (ln_g || ln_b) return fail(WM_E_ARG, "the K-long form has no LayerNorm prologue");
    } else if (!dec_linear_supports_k(K)) return fail(WM_E_ARG, "K must be a multiple of 32 whose k-steps split over <= 16 waves x <= 4 steps (K <= 2048), or 3072");
    if (!ln_g != !ln_b) return fail(WM_E_ARG, "ln_g and ln_b go together");
    if (ln_g && x_is_t) return fail(WM_E_ARG, "the LayerNorm prologue reads fp32 rows (no x_is_t)");
    if (!kcache != !vcache) return fail(WM_E_ARG, "kcache and vcache go together");
    if (out_is_t && (residual || kcache)) return fail(WM_E_ARG, "out_is_t is the plain store (no residual, no cache append)");
    const int d = N / 3;
    if (kcache) {
        if (N % 3 || d % 64 || kv_dtype < 0 || kv_dtype > 2 || n_utt <= 0 || cap_rows <= 0 || len < 0)
            return fail(WM_E_ARG, "QKV mode needs N = 3 * d_model (d_model % 64 == 0), a kv_dtype and a cache [n_utt][cap_rows][d_model]");
        if (residual) return fail(WM_E_ARG, "QKV mode has no residual");
        if (kv_B < 0 || (kv_B > 0 ? (kv_B > n_utt || B % kv_B || len + B / kv_B > cap_rows) : (B > n_utt || len + 1 > cap_rows)))
            return fail(WM_E_ARG, "rows must be P * kv_B with kv_B <= n_utt and len + P <= cap_rows, or <= n_utt with len < cap_rows");
    }
    if (cap && cap_map) {
        if (!cap_sel || cap_dst <= 0 || cap_nsel <= 0 || cap_nsel > 32 || N % 64 || N > 2048 || kcache)
            return fail(WM_E_ARG, "capture by row map needs cap_sel, cap_dst > 0, N = 64 * heads <= 2048, 1 <= cap_nsel <= 32 (and no cache)");
        for (int h = 0; h < 32; ++h)
            if (cap_sel[h] >= cap_nsel || (cap_sel[h] >= 0 && h >= N / 64)) return fail(WM_E_ARG, "cap_sel names a slot >= cap_nsel or a head >= N / 64");
        for (int r = 0; r < B; ++r)
            if (cap_map[r] < -1 || cap_map[r] >= cap_dst) return fail(WM_E_ARG, "cap_map[%d] = %d outside [-1, cap_dst = %d)", r, cap_map[r], cap_dst);
    } else if (cap) {
        if (!cap_sel || len < 0 || cap_steps <= 0 || cap_nsel <= 0 || cap_nsel > 32 || N % 64 || N > 2048 || (kcache && cap))
            return fail(WM_E_ARG, "capture needs cap_sel, len >= 0, N = 64 * heads <= 2048, 1 <= cap_nsel <= 32, cap_steps > 0 (and no cache)");
        for (int h = 0; h < 32; ++h)
            if (cap_sel[h] >= cap_nsel || (cap_sel[h] >= 0 && h >= N / 64)) return fail(WM_E_ARG, "cap_sel names a slot >= cap_nsel or a head >= N / 64");
    }
    TmpDev t;
    hipStream_t st = nullptr;
    // the kernel stores whole 16-column tiles (and loads the residual the same way): rows padded to 16 columns
    const int wout = kcache ? d : N, ldo = (wout + 15) / 16 * 16;
    const int odt = out_is_t ? dtype : WM_F32;
    const size_t ncache = kcache ? (size_t)n_utt * cap_rows * d : 0;
    const size_t ncap = !cap ? 0 : cap_map ? (size_t)cap_dst * cap_nsel * 64 : (size_t)B * cap_steps * cap_nsel * 64;
    DevBuf &dx = t.add(), &w = t.add(), &b = t.add(), &g = t.add(), &be = t.add(), &o = t.add(), &r = t.add(), &kc = t.add(), &vc = t.add(),
           &ctl = t.add(), &cp = t.add(), &cm = t.add();
    WMCHK(upload(dx, x, (size_t)B * K, x_is_t ? dtype : WM_F32));
    WMCHK(upload(w, W, (size_t)N * K, dtype));
    if (bias) WMCHK(upload(b, bias, N, WM_F32));
    if (ln_g) {
        WMCHK(upload(g, ln_g, K, WM_F32));
        WMCHK(upload(be, ln_b, K, WM_F32));
    }
    WMCHK(o.alloc((size_t)B * ldo * dt_size(odt), true));
    const bool in_place = residual == out;
    if (residual) {
        DevBuf& dst = in_place ? o : r;
        if (!in_place) WMCHK(r.alloc((size_t)B * ldo * 4, true));
        HIPCHK(hipMemcpy2D(dst.p, (size_t)ldo * 4, residual, (size_t)N * 4, (size_t)N * 4, B, hipMemcpyHostToDevice));
    }
    DecLinearParams p = linear_block(dx.as<float>(), ln_g ? g.as<float>() : nullptr, ln_g ? be.as<float>() : nullptr, w.p, bias ? b.as<float>() : nullptr,
                                     N, K, B, o.as<float>(), ldo);
    p.x_is_t = x_is_t;
    p.out_is_t = out_is_t;
    p.act = act != 0;
    p.gelu_mode = gelu_mode;
    p.residual = residual ? (in_place ? o.as<float>() : r.as<float>()) : nullptr;
    p.ldr = ldo;
    if (kcache || (cap && !cap_map)) {
        StepCtl h{};
        h.len = len;
        WMCHK(upload_bytes(ctl, &h, sizeof h));
        p.ctl = ctl.as<StepCtl>();
    }
    if (kcache) {
        WMCHK(upload(kc, kcache, ncache, kv_dtype));
        WMCHK(upload(vc, vcache, ncache, kv_dtype));
        p.kcache = kc.p;
        p.vcache = vc.p;
        p.kv_batch_stride = (long)((size_t)cap_rows * d);
        p.d_model = d;
        p.kv_dtype = kv_dtype;
        p.kv_B = kv_B;
    }
    if (cap) {
        WMCHK(upload(cp, cap, ncap, WM_F32));
        p.cap = cp.as<float>();
        p.cap_row_stride = (long)cap_steps * cap_nsel * 64;
        p.cap_step0 = cap_step0;
        p.cap_steps = cap_steps;
        p.cap_nsel = cap_nsel;
        memcpy(p.cap_sel, cap_sel, 32);
        if (cap_map) {
            WMCHK(upload_bytes(cm, cap_map, (size_t)B * 4));
            p.cap_map = cm.as<int>();
        }
    }
    WMCHK(dec_linear_dispatch(dtype, p, st));
    HIPCHK(hipGetLastError());
    WMCHK(download_f32_rows(out, o, B, wout, ldo, odt));
    if (kcache) {
        WMCHK(download_f32(kcache, kc, ncache, kv_dtype));
        WMCHK(download_f32(vcache, vc, ncache, kv_dtype));
    }
    if (cap) HIPCHK(hipMemcpy(cap, cp.p, ncap * 4, hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int wm_op_dec_linear(float* out, const float* x, const float* W, const float* bias, const float* ln_g, const float* ln_b,
                                const float* residual, int B, int N, int K, int dtype, int x_is_t, int out_is_t, int act, int gelu_mode,
                                float* kcache, float* vcache, int n_utt, int cap_rows, int kv_dtype, int kv_B, int len, float* cap,
                                const int8_t* cap_sel, int cap_step0, int cap_steps, int cap_nsel) {
    return op_dec_linear(out, x, W, bias, ln_g, ln_b, residual, B, N, K, dtype, x_is_t, out_is_t, act, gelu_mode, kcache, vcache, n_utt, cap_rows,
                         kv_dtype, kv_B, len, cap, cap_sel, cap_step0, cap_steps, cap_nsel);
}
// The K-long form of the same launch (fc2 of d_model 768 / 1024): K = 3072 or 4096, no LayerNorm prologue.  wm_op_dec_linear keeps
// refusing K = 4096; K = 3072 runs the same kernel through either hook.
extern "C" int wm_op_dec_linear_long(float* out, const float* x, const float* W, const float* bias, const float* ln_g, const float* ln_b,
                                     const float* residual, int B, int N, int K, int dtype, int x_is_t, int out_is_t, int act, int gelu_mode,
                                     float* kcache, float* vcache, int n_utt, int cap_rows, int kv_dtype, int kv_B, int len, float* cap,
                                     const int8_t* cap_sel, int cap_step0, int cap_steps, int cap_nsel) {
    return op_dec_linear(out, x, W, bias, ln_g, ln_b, residual, B, N, K, dtype, x_is_t, out_is_t, act, gelu_mode, kcache, vcache, n_utt, cap_rows,
                         kv_dtype, kv_B, len, cap, cap_sel, cap_step0, cap_steps, cap_nsel, nullptr, 0, true);
}
// LNx -> cross q as an align pass wires it: B input rows, cap [cap_dst][cap_nsel][64] in and out, cap_map [B] in [-1, cap_dst)
extern "C" int wm_op_dec_linear_capmap(float* out, float* cap, const float* x, const float* W, const float* bias, const float* ln_g,
                                       const float* ln_b, int B, int N, int K, int dtype, const int8_t* cap_sel, int cap_nsel,
                                       const int32_t* cap_map, int cap_dst) {
    if (!cap || !cap_map) return fail(WM_E_ARG, "bad argument");
    return op_dec_linear(out, x, W, bias, ln_g, ln_b, nullptr, B, N, K, dtype, 0, 0, 0, 0, nullptr, nullptr, 0, 0, 0, 0, 0, cap, cap_sel, 0, 0,
                         cap_nsel, cap_map, cap_dst);
}

// The decode step's final LayerNorm + tied-embedding logits and its fused argmax, wired as decode_core (Logits::full) and
// argmax_peek wire them: launch_dec_logits picks the kernel variant from (dtype, K, B), argmax_step reduces its partials.
// logprob non-null: the LP instantiation of the same kernel variant, and the chosen ids' log-probabilities [B] (wm_op_logits_lp)
static int op_logits(float* logits, int32_t* ids, float* logprob, const float* x, const float* ln_g, const float* ln_b, const float* emb,
                     const float* mask, const int32_t* ranges, int timestamp_begin, int B, int N, int K, int dtype, const uint32_t* seen = nullptr,
                     const uint32_t* ban = nullptr, float penalty = 1.f, const uint32_t* hit = nullptr, const int32_t* slot_id = nullptr,
                     int n_slots = 0, const float* slot_bias = nullptr, const int32_t* slot_flags = nullptr, int top_k = 0,
                     int32_t* top_ids = nullptr, float* top_lp = nullptr) {
    if (!logits || !ids || !x || !ln_g || !ln_b || !emb || B <= 0 || N <= 0) return fail(WM_E_ARG, "bad argument");
    if (top_k && (top_k < 1 || top_k > TOPK_MAX || !logprob || !top_ids || !top_lp)) return fail(WM_E_ARG, "top_k must be 1..%d, with the log-prob outputs", TOPK_MAX);
    WMCHK(vocab_k_check(K));
    if (dtype < 0 || dtype > 2) return fail(WM_E_ARG, "bad dtype");
    if (ranges && (timestamp_begin <= 0 || timestamp_begin >= N)) return fail(WM_E_ARG, "ranges need 0 < timestamp_begin < N");
    TmpDev t;
    hipStream_t st = nullptr;
    const int ldo = (N + 3) / 4 * 4, npart = dec_logits_parts(N);  // the kernel stores whole float4 groups below ldo
    const float* dx;
    VocabHead vh;
    WMCHK(upload_vocab_head(t, x, ln_g, ln_b, emb, B, N, K, dtype, &dx, &vh));
    DevBuf &mk = t.add(), &o = t.add(), &av = t.add(), &ai = t.add(), &tst = t.add(), &tv = t.add(), &ti = t.add(), &tm = t.add(), &ts = t.add(),
           &nx = t.add(), &ls = t.add(), &ln = t.add();
    if (mask) WMCHK(upload(mk, mask, N, WM_F32));
    WMCHK(o.alloc((size_t)B * ldo * 4, true));
    WMCHK(av.alloc((size_t)B * npart * 4, true));
    WMCHK(ai.alloc((size_t)B * npart * 4, true));
    WMCHK(nx.alloc((size_t)B * 4, true));
    if (logprob) {
        WMCHK(ls.alloc((size_t)B * npart * 4, true));
        WMCHK(ln.alloc((size_t)B * 4, true));
    }
    TsRules rules{};
    if (ranges) {
        std::vector<TsState> h(B);
        for (int b = 0; b < B; ++b) {
            h[b] = TsState{};
            h[b].n_gen = 1;
            h[b].t_last = -1;
            h[b].text_lo = ranges[4 * b];
            h[b].text_hi = ranges[4 * b + 1];
            h[b].ts_lo = ranges[4 * b + 2];
            h[b].ts_hi = ranges[4 * b + 3];
        }
        WMCHK(upload_bytes(tst, h.data(), (size_t)B * sizeof(TsState)));
        for (DevBuf* d : {&tv, &ti, &tm, &ts}) WMCHK(d->alloc((size_t)B * npart * 4, true));
        rules.tb = timestamp_begin;
        rules.eos = timestamp_begin;
        rules.max_init = -1;
        rules.vocab = N;
    }
    DecLinearParams p = linear_block(dx, vh.ln_g, vh.ln_b, vh.emb, nullptr, N, K, B, o.as<float>(), ldo);
    p.amax_val = av.as<float>();
    p.amax_idx = ai.as<int>();
    p.amax_stride = npart;
    p.amax_mask = mask ? mk.as<float>() : nullptr;
    if (ranges) {
        p.ts_state = tst.as<TsState>();
        p.ts_begin = timestamp_begin;
        p.ts_val = tv.as<float>();
        p.ts_idx = ti.as<int>();
        p.ts_m = tm.as<float>();
        p.ts_s = ts.as<float>();
    }
    if (logprob) p.lp_s = ls.as<float>();
    if (seen) {  // wm_op_logits_processed: the rows' sets as given, the RP instantiation of the same kernel variant
        DevBuf &ds = t.add(), &db = t.add(), &dc = t.add();
        const size_t words = (size_t)repeat_words(N);
        const RepeatCtl ctl{penalty, 0};
        WMCHK(upload_bytes(ds, seen, B * words * 4));
        WMCHK(upload_bytes(db, ban, B * words * 4));
        WMCHK(upload_bytes(dc, &ctl, sizeof(ctl)));
        p.rp_seen = ds.as<unsigned>();
        p.rp_ban = db.as<unsigned>();
        p.rp_ctl = dc.as<RepeatCtl>();
        p.rp_words = (int)words;
        if (hit) {  // wm_op_logits_seq_bias: the rows' hit bits and slots as given, the SB instantiation of the same kernel variant
            DevBuf &dh = t.add(), &dv = t.add(), &di = t.add(), &dt = t.add();
            std::vector<int32_t> h_of((size_t)N, -1);
            for (int k = 0; k < n_slots; ++k) h_of[slot_id[k]] = k;
            std::vector<SeqSlot> h((size_t)B * SEQ_BIAS_MAX, SeqSlot{0.f, 0});
            for (int b = 0; b < B; ++b)
                for (int k = 0; k < n_slots; ++k) h[(size_t)b * SEQ_BIAS_MAX + k] = SeqSlot{slot_bias[(size_t)b * n_slots + k], slot_flags[(size_t)b * n_slots + k]};
            SeqBiasCtl sc{};
            sc.n_slots = n_slots;
            sc.eot = -1;
            WMCHK(upload_bytes(dh, hit, B * words * 4));
            WMCHK(upload_bytes(dv, h.data(), h.size() * sizeof(SeqSlot)));
            WMCHK(upload_bytes(di, h_of.data(), (size_t)N * 4));
            sc.slot_of = di.as<int>();
            WMCHK(upload_bytes(dt, &sc, sizeof(sc)));
            p.sb_hit = dh.as<unsigned>();
            p.sb_val = dv.as<SeqSlot>();
            p.sb_ctl = dt.as<SeqBiasCtl>();
        }
    }
    int lrc = 0;
    DISPATCH_DT(dtype, TT, lrc = launch_dec_logits<TT>(p, st));
    LCHK(lrc);
    ArgmaxParams a{};
    if (logprob) {
        a.lp_s = ls.as<float>();
        a.lp_next = ln.as<float>();
    }
    DevBuf &kr = t.add(), &ki = t.add(), &kl = t.add();  // wm_op_logits_topk: the rows' TopkRow and the [B][k] tables (slot = row)
    if (top_k) {
        WMCHK(kr.alloc((size_t)B * sizeof(TopkRow), true));
        WMCHK(ki.alloc((size_t)B * top_k * 4, true));
        WMCHK(kl.alloc((size_t)B * top_k * 4, true));
        a.tk_rows = kr.as<TopkRow>();
    }
    if (ranges) {
        a.ts_state = tst.as<TsState>();
        a.rules = rules;
        a.ts_val = tv.as<float>();
        a.ts_idx = ti.as<int>();
        a.ts_m = tm.as<float>();
        a.ts_s = ts.as<float>();
        a.ts_part0 = timestamp_begin / dec_logits_ids_per_part(N);
    }
    a.logits = o.as<float>();
    a.ldl = ldo;
    a.V = N;
    a.B = B;
    a.pval = av.as<float>();
    a.pidx = ai.as<int>();
    a.npart = npart;
    a.next = nx.as<int>();
    LCHK(launch_argmax_step(a, st));
    if (top_k) {  // the selection launch as topk_select wires it behind the step's argmax
        TopkSelectParams q{};
        q.logits = o.as<float>();
        q.ldl = ldo;
        q.V = N;
        q.B = B;
        q.mask = p.amax_mask;
        q.rows = kr.as<TopkRow>();
        q.k = top_k;
        q.ids = ki.as<int>();
        q.lps = kl.as<float>();
        LCHK(launch_topk_select(q, st));
    }
    HIPCHK(hipGetLastError());
    WMCHK(download_f32_rows(logits, o, B, N, ldo, WM_F32));
    if (top_k) {
        HIPCHK(hipMemcpy(top_ids, ki.p, (size_t)B * top_k * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(top_lp, kl.p, (size_t)B * top_k * 4, hipMemcpyDeviceToHost));
    }
    HIPCHK(hipMemcpy(ids, nx.p, (size_t)B * 4, hipMemcpyDeviceToHost));
    if (logprob) HIPCHK(hipMemcpy(logprob, ln.p, (size_t)B * 4, hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int wm_op_logits(float* logits, int32_t* ids, const float* x, const float* ln_g, const float* ln_b, const float* emb,
                            const float* mask, const int32_t* ranges, int timestamp_begin, int B, int N, int K, int dtype) {
    return op_logits(logits, ids, nullptr, x, ln_g, ln_b, emb, mask, ranges, timestamp_begin, B, N, K, dtype);
}
extern "C" int wm_op_logits_lp(float* logits, int32_t* ids, float* logprob, const float* x, const float* ln_g, const float* ln_b, const float* emb,
                               const float* mask, const int32_t* ranges, int timestamp_begin, int B, int N, int K, int dtype) {
    if (!logprob) return fail(WM_E_ARG, "bad argument");
    return op_logits(logits, ids, logprob, x, ln_g, ln_b, emb, mask, ranges, timestamp_begin, B, N, K, dtype);
}
// The same two launches with the repetition processors on given sets: seen / ban [B][ceil(N / 32)], bit (id & 31) of word
// id >> 5.  logprob null: the instantiation without log-probabilities.
extern "C" int wm_op_logits_processed(float* logits, int32_t* ids, float* logprob, const float* x, const float* ln_g, const float* ln_b,
                                      const float* emb, const float* mask, const int32_t* ranges, int timestamp_begin, const uint32_t* seen,
                                      const uint32_t* ban, float penalty, int B, int N, int K, int dtype) {
    if (!seen || !ban || !(penalty > 0.f)) return fail(WM_E_ARG, "bad argument");
    return op_logits(logits, ids, logprob, x, ln_g, ln_b, emb, mask, ranges, timestamp_begin, B, N, K, dtype, seen, ban, penalty);
}
// The same launches with the top-k alternatives: the TK instantiation of argmax_step and the selection launch behind it, on
// arbitrary rows, masks and ranges; seen / ban (both or neither, with penalty) add the repetition processors.  top_ids / top_lp [B][k].
extern "C" int wm_op_logits_topk(float* logits, int32_t* ids, float* logprob, int32_t* top_ids, float* top_lp, int top_k, const float* x,
                                 const float* ln_g, const float* ln_b, const float* emb, const float* mask, const int32_t* ranges,
                                 int timestamp_begin, const uint32_t* seen, const uint32_t* ban, float penalty, int B, int N, int K, int dtype) {
    if (!logprob || !top_ids || !top_lp || top_k < 1 || (!seen != !ban) || (seen && !(penalty > 0.f))) return fail(WM_E_ARG, "bad argument");
    return op_logits(logits, ids, logprob, x, ln_g, ln_b, emb, mask, ranges, timestamp_begin, B, N, K, dtype, seen, ban, penalty, nullptr, nullptr, 0,
                     nullptr, nullptr, top_k, top_ids, top_lp);
}
// Forced-token replay, shared by wm_op_repeat_sets, wm_op_seq_bias_hits and wm_op_constraint_states: repeat_init on each row's prompt tokens[b][0 ..
// prompt_len[b]), then one argmax launch per step that is handed the row's next id of the table as its only candidate, so it appends
// exactly that id — rows end at n_ids[b] (a row past its end is `finished` and does nothing).
static int replay_rows_check(const int32_t* tokens, const int32_t* prompt_len, const int32_t* n_ids, int B, int stride, int vocab) {
    for (int b = 0; b < B; ++b) {
        if (prompt_len[b] < 1 || prompt_len[b] > n_ids[b] || n_ids[b] > stride) return fail(WM_E_ARG, "row %d: need 1 <= prompt_len <= n_ids <= stride", b);
        for (int i = 0; i < n_ids[b]; ++i)
            if (tokens[(size_t)b * stride + i] < 0 || tokens[(size_t)b * stride + i] >= vocab) return fail(WM_E_ARG, "token id out of range");
    }
    return 0;
}
// extra: the hook's own fields of every step's ArgmaxParams (ArgmaxCtParams: the constrained launch).  init(r): the hook's launch behind repeat_init, on the same prompt
// buffers.  fetch(s, seen, ban): copies entry s out — 0 after the init, s after step s.
template <typename Params, typename Init, typename Fetch>
static int replay_forced(TmpDev& t, const int32_t* tokens, const int32_t* prompt_len, const int32_t* n_ids, int B, int stride, int vocab, int ngram,
                         int steps, const Params& extra, Init init, Fetch fetch) {
    hipStream_t st = nullptr;
    const size_t words = (size_t)repeat_words(vocab), set_bytes = (size_t)B * words * 4;
    DevBuf &ds = t.add(), &db = t.add(), &dc = t.add(), &out = t.add(), &nt = t.add(), &fin = t.add(), &ctl = t.add(), &pv = t.add(), &pi = t.add(),
           &nx = t.add(), &pos = t.add();
    WMCHK(ds.alloc(set_bytes));
    WMCHK(db.alloc(set_bytes));
    WMCHK(dc.alloc(sizeof(RepeatCtl)));
    WMCHK(fin.alloc((size_t)B * 4, true));
    WMCHK(ctl.alloc(sizeof(StepCtl), true));
    WMCHK(pv.alloc((size_t)B * 4, true));  // one partial per row: value 0, index = the id to append
    WMCHK(pi.alloc((size_t)B * 4));
    WMCHK(nx.alloc((size_t)B * 4));
    WMCHK(pos.alloc((size_t)B * 4, true));
    std::vector<int32_t> h_out((size_t)B * stride, 0), h_idx(B), h_fin(B);
    for (int b = 0; b < B; ++b) std::copy(tokens + (size_t)b * stride, tokens + (size_t)b * stride + prompt_len[b], h_out.begin() + (size_t)b * stride);
    WMCHK(upload_bytes(out, h_out.data(), h_out.size() * 4));
    WMCHK(upload_bytes(nt, prompt_len, (size_t)B * 4));
    RepeatInitParams r{};
    r.seen = ds.as<unsigned>();
    r.ban = db.as<unsigned>();
    r.words = (int)words;
    r.B = B;
    r.ctl = dc.as<RepeatCtl>();
    r.penalty = 1.f;
    r.ngram = ngram;
    r.out_tokens = out.as<int>();
    r.out_stride = stride;
    r.n_tokens = nt.as<int>();
    launch_repeat_init(r, st);
    WMCHK(init(r));
    HIPCHK(hipGetLastError());
    WMCHK(fetch(0, ds, db));
    for (int s = 1; s <= steps; ++s) {
        for (int b = 0; b < B; ++b) {
            const int at = prompt_len[b] + s - 1;
            h_fin[b] = at >= n_ids[b];
            h_idx[b] = h_fin[b] ? 0 : tokens[(size_t)b * stride + at];
        }
        HIPCHK(hipMemcpy(pi.p, h_idx.data(), (size_t)B * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(fin.p, h_fin.data(), (size_t)B * 4, hipMemcpyHostToDevice));
        Params a = extra;
        a.V = vocab;
        a.B = B;
        a.pval = pv.as<float>();
        a.pidx = pi.as<int>();
        a.npart = 1;
        a.next = nx.as<int>();
        a.out_tokens = out.as<int>();
        a.out_stride = stride;
        a.n_tokens = nt.as<int>();
        a.finished = fin.as<int>();
        a.ctl = ctl.as<StepCtl>();
        a.pos = pos.as<int>();
        a.eot = -1;
        a.ignore_eot = 1;
        a.rp_seen = ds.as<unsigned>();
        a.rp_ban = db.as<unsigned>();
        a.rp_ctl = dc.as<RepeatCtl>();
        a.rp_words = (int)words;
        if constexpr (std::is_same<Params, ArgmaxCtParams>::value)
            LCHK(launch_argmax_step_ct(a, st));
        else
            LCHK(launch_argmax_step(a, st));
        HIPCHK(hipGetLastError());
        WMCHK(fetch(s, ds, db));
    }
    return 0;
}
// The sets' bookkeeping alone, replayed.  seen / ban: [steps + 1][B][ceil(vocab / 32)], entry 0 after the init, entry s after step s.
extern "C" int wm_op_repeat_sets(uint32_t* seen, uint32_t* ban, const int32_t* tokens, const int32_t* prompt_len, const int32_t* n_ids, int B,
                                 int stride, int vocab, int ngram, int steps) {
    if (!seen || !ban || !tokens || !prompt_len || !n_ids || B <= 0 || stride <= 0 || vocab <= 0 || steps < 0) return fail(WM_E_ARG, "bad argument");
    if (ngram < 0 || ngram > REPEAT_NGRAM_MAX) return fail(WM_E_ARG, "no_repeat_ngram_size %d outside [0, %d]", ngram, REPEAT_NGRAM_MAX);
    WMCHK(replay_rows_check(tokens, prompt_len, n_ids, B, stride, vocab));
    TmpDev t;
    const size_t set_words = (size_t)B * repeat_words(vocab);
    auto fetch = [&](int s, const DevBuf& ds, const DevBuf& db) -> int {
        HIPCHK(hipMemcpy(seen + s * set_words, ds.p, set_words * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(ban + s * set_words, db.p, set_words * 4, hipMemcpyDeviceToHost));
        return 0;
    };
    return replay_forced(t, tokens, prompt_len, n_ids, B, stride, vocab, ngram, steps, ArgmaxParams{}, [](const RepeatInitParams&) { return 0; }, fetch);
}
// The same two launches with sequence bias / bad words on given hit state: hit [B][ceil(N / 32)], the slots' ids
// (ascending) and, per row and slot, the summed bias and the flags (bit 0 on, bit 1 ban).  seen / ban / penalty as above.
extern "C" int wm_op_logits_seq_bias(float* logits, int32_t* ids, float* logprob, const float* x, const float* ln_g, const float* ln_b,
                                     const float* emb, const float* mask, const int32_t* ranges, int timestamp_begin, const uint32_t* seen,
                                     const uint32_t* ban, float penalty, const uint32_t* hit, const int32_t* slot_id, int n_slots,
                                     const float* slot_bias, const int32_t* slot_flags, int B, int N, int K, int dtype) {
    if (!seen || !ban || !(penalty > 0.f) || !hit || !slot_id || !slot_bias || !slot_flags || n_slots < 1 || n_slots > SEQ_BIAS_MAX)
        return fail(WM_E_ARG, "bad argument");
    for (int k = 0; k < n_slots; ++k)
        if (slot_id[k] < 0 || slot_id[k] >= N || (k && slot_id[k] <= slot_id[k - 1])) return fail(WM_E_ARG, "slot ids must ascend inside the vocabulary");
    // the kernel looks a set bit's slot up without a check (the drivers set a bit only for a slot's id): refuse any other bit here
    if (B > 0 && N > 0) {
        std::vector<char> is_slot((size_t)N, 0);
        for (int k = 0; k < n_slots; ++k) is_slot[slot_id[k]] = 1;
        const int words = repeat_words(N);
        for (int b = 0; b < B; ++b)
            for (int t = 0; t < words * 32; ++t)
                if ((hit[(size_t)b * words + (t >> 5)] >> (t & 31) & 1u) && (t >= N || !is_slot[t])) return fail(WM_E_ARG, "row %d: hit bit %d has no slot", b, t);
    }
    return op_logits(logits, ids, logprob, x, ln_g, ln_b, emb, mask, ranges, timestamp_begin, B, N, K, dtype, seen, ban, penalty, hit, slot_id, n_slots,
                     slot_bias, slot_flags);
}
// The hit state's bookkeeping alone, as wm_op_repeat_sets runs the sets': seq_bias_init on each row's prompt, then one argmax launch
// per step that appends the row's next id of the table.  The table is built from the two lists as wm_set_sequence_bias builds it (same
// refusals).  slot_id [n_seq + n_bad] and *n_slots: the table's slots; hit [steps + 1][B][ceil(vocab / 32)], slot_bias / slot_flags
// [steps + 1][B][n_seq + n_bad] (the first *n_slots of each row are written) — entry 0 after the init, entry s after step s.
extern "C" int wm_op_seq_bias_hits(uint32_t* hit, float* slot_bias, int32_t* slot_flags, int32_t* slot_id, int32_t* n_slots, const int32_t* tokens,
                                   const int32_t* prompt_len, const int32_t* n_ids, int B, int stride, int vocab, int eot, const int32_t* seq_ids,
                                   const int32_t* seq_off, const float* seq_bias, int n_seq, const int32_t* bad_ids, const int32_t* bad_off, int n_bad,
                                   int steps) {
    if (!hit || !slot_bias || !slot_flags || !slot_id || !n_slots || !tokens || !prompt_len || !n_ids || B <= 0 || stride <= 0 || vocab <= 0 || steps < 0)
        return fail(WM_E_ARG, "bad argument");
    WMCHK(replay_rows_check(tokens, prompt_len, n_ids, B, stride, vocab));
    std::shared_ptr<SeqTable> tab;
    std::vector<int32_t> sid;
    WMCHK(build_seq_table(tab, vocab, seq_ids, seq_off, seq_bias, n_seq, bad_ids, bad_off, n_bad, &sid));
    if (!tab) return fail(WM_E_ARG, "both lists are empty");
    const int cap = n_seq + n_bad, ns = tab->n_slots;
    *n_slots = ns;
    std::copy(sid.begin(), sid.end(), slot_id);
    TmpDev t;
    const size_t words = (size_t)repeat_words(vocab), set_bytes = (size_t)B * words * 4;
    DevBuf &dh = t.add(), &dv = t.add(), &dsc = t.add();
    WMCHK(dh.alloc(set_bytes));
    WMCHK(dv.alloc((size_t)B * SEQ_BIAS_MAX * sizeof(SeqSlot), true));
    WMCHK(dsc.alloc(sizeof(SeqBiasCtl)));
    ArgmaxParams extra{};
    extra.sb_hit = dh.as<unsigned>();
    extra.sb_val = dv.as<SeqSlot>();
    extra.sb_ctl = dsc.as<SeqBiasCtl>();
    auto init = [&](const RepeatInitParams& r) -> int {
        SeqBiasInitParams q{};
        q.hit = dh.as<unsigned>();
        q.val = dv.as<SeqSlot>();
        q.words = (int)words;
        q.B = B;
        q.ctl = dsc.as<SeqBiasCtl>();
        q.table = tab->ctl(eot);
        q.out_tokens = r.out_tokens;
        q.out_stride = stride;
        q.n_tokens = r.n_tokens;
        LCHK(launch_seq_bias_init(q, nullptr));
        return 0;
    };
    std::vector<SeqSlot> h_val((size_t)B * SEQ_BIAS_MAX);
    auto fetch = [&](int s, const DevBuf&, const DevBuf&) -> int {
        HIPCHK(hipMemcpy(hit + (size_t)s * B * words, dh.p, set_bytes, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(h_val.data(), dv.p, h_val.size() * sizeof(SeqSlot), hipMemcpyDeviceToHost));
        for (int b = 0; b < B; ++b)
            for (int k = 0; k < ns; ++k) {
                slot_bias[((size_t)s * B + b) * cap + k] = h_val[(size_t)b * SEQ_BIAS_MAX + k].bias;
                slot_flags[((size_t)s * B + b) * cap + k] = h_val[(size_t)b * SEQ_BIAS_MAX + k].flags;
            }
        return 0;
    };
    return replay_forced(t, tokens, prompt_len, n_ids, B, stride, vocab, 0, steps, extra, init, fetch);
}
// The phrase-list constraint's bookkeeping alone, replayed likewise: constraint_init behind the repeat init on each row's
// prompt, then one argmax launch per step that appends the row's next id of the table.  The table is built from the phrases as
// wm_set_constraint builds it (same refusals; eot: allowed where a phrase ends, refused inside one).  node [steps + 1][B] and mask
// [steps + 1][B][ceil(vocab / 32)], the rows' `ban` words — entry 0 after the init, entry s after step s.
extern "C" int wm_op_constraint_states(int32_t* node, uint32_t* mask, const int32_t* tokens, const int32_t* prompt_len, const int32_t* n_ids, int B,
                                       int stride, int vocab, int eot, int ngram, const int32_t* ids, const int32_t* offsets, int n_phrases,
                                       int free_from, int steps) {
    if (!node || !mask || !tokens || !prompt_len || !n_ids || B <= 0 || stride <= 0 || vocab <= 0 || steps < 0) return fail(WM_E_ARG, "bad argument");
    if (ngram < 0 || ngram > REPEAT_NGRAM_MAX) return fail(WM_E_ARG, "no_repeat_ngram_size %d outside [0, %d]", ngram, REPEAT_NGRAM_MAX);
    WMCHK(replay_rows_check(tokens, prompt_len, n_ids, B, stride, vocab));
    std::shared_ptr<ConstraintTable> tab;
    WMCHK(build_constraint_table(tab, vocab, ids, offsets, n_phrases, free_from));
    if (!tab) return fail(WM_E_ARG, "the list of phrases is empty");
    if (tab->holds(eot)) return fail(WM_E_ARG, "constraint: a phrase holds the eot %d", eot);
    TmpDev t;
    const size_t words = (size_t)repeat_words(vocab), set_bytes = (size_t)B * words * 4;
    DevBuf &dn = t.add(), &dm = t.add(), &dcc = t.add();
    WMCHK(dn.alloc((size_t)B * 4, true));
    WMCHK(dm.alloc((size_t)B * 4, true));
    WMCHK(dcc.alloc(sizeof(ConstraintCtl)));
    ArgmaxCtParams extra{};
    extra.ct_node = dn.as<int>();
    extra.ct_match = dm.as<int>();
    extra.ct_ctl = dcc.as<ConstraintCtl>();
    auto init = [&](const RepeatInitParams& r) -> int {
        ConstraintInitParams q{};
        q.ban = r.ban;
        q.seen = r.seen;
        q.words = (int)words;
        q.B = B;
        q.vocab = vocab;
        q.node = dn.as<int>();
        q.match = dm.as<int>();
        q.ctl = dcc.as<ConstraintCtl>();
        q.table = tab->ctl(eot);
        q.ngram = ngram;
        q.out_tokens = r.out_tokens;
        q.out_stride = stride;
        q.n_tokens = r.n_tokens;
        LCHK(launch_constraint_init(q, nullptr));
        return 0;
    };
    auto fetch = [&](int s, const DevBuf&, const DevBuf& db) -> int {
        HIPCHK(hipMemcpy(node + (size_t)s * B, dn.p, (size_t)B * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(mask + (size_t)s * B * words, db.p, set_bytes, hipMemcpyDeviceToHost));
        return 0;
    };
    return replay_forced(t, tokens, prompt_len, n_ids, B, stride, vocab, ngram, steps, extra, init, fetch);
}

// ---- the pass-control kernels and the timestamp rules' state machine ---------------------------------------------
// The start of a pass on device buffers that already hold the caller's values: launch_init_tokens (len null: the shared prompt
// prompt[0 .. n_prompt), at most 16 ids) or launch_init_tokens_rows (row b's prompt prompt[b * row_stride .. + len[b]), Lmax cache rows).
// Shared by wm_op_init_tokens and wm_op_ts_states; the arguments are checked by the callers.
struct InitDev {
    int *out_tokens, *n_tokens, *finished, *tok_rows, *pos_rows, *key_lo;
    StepCtl* ctl;
    TsState* ts_state;
    float *logprobs, *lp_sum;
};
static int op_launch_init(TmpDev& t, const InitDev& d, const int32_t* prompt, int n_prompt, const int32_t* len, int row_stride, int Lmax, int B,
                          int out_stride, const TsRules& rules) {
    InitTokensParams ip{};
    ip.out_tokens = d.out_tokens;
    ip.out_stride = out_stride;
    ip.n_tokens = d.n_tokens;
    ip.finished = d.finished;
    ip.ctl = d.ctl;
    ip.B = B;
    ip.tok_rows = d.tok_rows;
    ip.pos_rows = d.pos_rows;
    ip.ts_state = d.ts_state;
    ip.rules = rules;
    ip.logprobs = d.logprobs;
    ip.lp_sum = d.lp_sum;
    if (!len) {
        ip.n_prompt = n_prompt;
        std::copy(prompt, prompt + n_prompt, ip.prompt);
        launch_init_tokens(ip, nullptr);
    } else {
        DevBuf &tab = t.add(), &dl = t.add();
        WMCHK(upload_bytes(tab, prompt, (size_t)B * row_stride * 4));
        WMCHK(upload_bytes(dl, len, (size_t)B * 4));
        launch_init_tokens_rows(ip, RowPromptParams{tab.as<int>(), dl.as<int>(), row_stride, Lmax, d.key_lo}, nullptr);
    }
    HIPCHK(hipGetLastError());
    return 0;
}
static int ts_rules_check(int vocab, int timestamp_begin, int eos) {
    if (timestamp_begin <= 0 || timestamp_begin >= vocab) return fail(WM_E_ARG, "timestamp rules need 0 < timestamp_begin < vocab");
    if (eos < 0 || eos > timestamp_begin) return fail(WM_E_ARG, "timestamp rules need 0 <= eos <= timestamp_begin");
    return 0;
}
// an in-and-out host array on the device, and back
static int up_opt(DevBuf& b, const void* h, size_t bytes) { return h ? upload_bytes(b, h, bytes) : 0; }
static int down_opt(void* h, const DevBuf& b, size_t bytes) {
    if (h) HIPCHK(hipMemcpy(h, b.p, bytes, hipMemcpyDeviceToHost));
    return 0;
}

// launch_init_tokens or launch_init_tokens_rows alone, one launch.  Every output array goes up with the caller's values and comes back
// whole.  len null: the shared prompt; else the rows form.  The row arrays hold B_held >= B rows and tok_rows / pos_rows rows_held
// position rows of B, so the caller sees what a thread past B or a slot past the prompt would have written.
extern "C" int wm_op_init_tokens(int32_t* out_tokens, int32_t* n_tokens, int32_t* finished, int32_t* ctl, int32_t* tok_rows, int32_t* pos_rows,
                                 int32_t* ts_state, float* logprobs, float* lp_sum, int32_t* key_lo, const int32_t* prompt, int n_prompt,
                                 const int32_t* len, int row_stride, int Lmax, int rows_held, int B, int B_held, int out_stride, int vocab,
                                 int timestamp_begin, int eos, int max_initial) {
    if (!out_tokens || !n_tokens || !finished || !ctl || !prompt || B <= 0 || B_held < B || B_held > (1 << 20) || out_stride <= 0 || out_stride > (1 << 16))
        return fail(WM_E_ARG, "bad argument");
    if (!tok_rows != !pos_rows || !logprobs != !lp_sum) return fail(WM_E_ARG, "tok_rows and pos_rows go together, and so do logprobs and lp_sum");
    int need_rows;
    if (!len) {
        if (n_prompt < 1 || n_prompt > 16 || n_prompt > out_stride) return fail(WM_E_ARG, "the shared prompt holds 1 .. 16 ids and fits out_stride");
        if (key_lo) return fail(WM_E_ARG, "key_lo belongs to the rows form");
        need_rows = n_prompt;
    } else {
        if (!tok_rows || !key_lo) return fail(WM_E_ARG, "the rows form needs tok_rows, pos_rows and key_lo");
        if (row_stride <= 0 || row_stride > (1 << 16) || Lmax < 1 || Lmax > row_stride) return fail(WM_E_ARG, "the rows form needs 1 <= Lmax <= row_stride");
        for (int b = 0; b < B; ++b)
            if (len[b] < 1 || len[b] > Lmax || len[b] > out_stride) return fail(WM_E_ARG, "row %d: need 1 <= len <= Lmax and len <= out_stride", b);
        need_rows = Lmax;
    }
    if (tok_rows && (rows_held < need_rows || rows_held > (1 << 16))) return fail(WM_E_ARG, "tok_rows / pos_rows hold fewer position rows than the prompt");
    TsRules rules{};
    if (ts_state) {
        WMCHK(ts_rules_check(vocab, timestamp_begin, eos));
        rules = TsRules{timestamp_begin, eos, max_initial, vocab};
    }
    TmpDev t;
    DevBuf &o = t.add(), &nt = t.add(), &fin = t.add(), &dc = t.add(), &tr = t.add(), &pr = t.add(), &ts = t.add(), &lp = t.add(), &ls = t.add(),
           &kl = t.add();
    const size_t nb = (size_t)B_held * 4, no = (size_t)B_held * out_stride * 4, nr = (size_t)std::max(rows_held, 0) * B * 4;
    WMCHK(upload_bytes(o, out_tokens, no));
    WMCHK(upload_bytes(nt, n_tokens, nb));
    WMCHK(upload_bytes(fin, finished, nb));
    WMCHK(upload_bytes(dc, ctl, sizeof(StepCtl)));
    WMCHK(up_opt(tr, tok_rows, nr));
    WMCHK(up_opt(pr, pos_rows, nr));
    WMCHK(up_opt(ts, ts_state, (size_t)B_held * sizeof(TsState)));
    WMCHK(up_opt(lp, logprobs, no));
    WMCHK(up_opt(ls, lp_sum, nb));
    WMCHK(up_opt(kl, key_lo, nb));
    InitDev d{o.as<int>(), nt.as<int>(), fin.as<int>(), tok_rows ? tr.as<int>() : nullptr, tok_rows ? pr.as<int>() : nullptr, kl.as<int>(),
              dc.as<StepCtl>(), ts_state ? ts.as<TsState>() : nullptr, logprobs ? lp.as<float>() : nullptr, logprobs ? ls.as<float>() : nullptr};
    WMCHK(op_launch_init(t, d, prompt, n_prompt, len, row_stride, Lmax, B, out_stride, rules));
    WMCHK(down_opt(out_tokens, o, no));
    WMCHK(down_opt(n_tokens, nt, nb));
    WMCHK(down_opt(finished, fin, nb));
    WMCHK(down_opt(ctl, dc, sizeof(StepCtl)));
    WMCHK(down_opt(tok_rows, tr, nr));
    WMCHK(down_opt(pos_rows, pr, nr));
    WMCHK(down_opt(ts_state, ts, (size_t)B_held * sizeof(TsState)));
    WMCHK(down_opt(logprobs, lp, no));
    WMCHK(down_opt(lp_sum, ls, nb));
    return down_opt(key_lo, kl, nb);
}

// Forced-token replay of the timestamp rules: the real init launch (row_prompts == 0: launch_init_tokens on the prompt all rows share;
// else launch_init_tokens_rows on the ragged rows, Lmax = max prompt_len), the launch that ends the prefill (launch_set_step /
// launch_set_rows_step: cache length and positions), then one launch_argmax_step per step with ts_state, rules and advance set.  Each
// launch gets the row's next id as its only candidate — a text id (< timestamp_begin) as the one text partial with no timestamp mass
// (ts_s = 0, ts_val = ts_m = -inf), a timestamp id as the one timestamp partial (value 0, mass 1) with no text candidate (index
// INT_MAX, value -inf) — so the kernel's own decision block picks it and its own history update runs.  A row past n_ids[b] is
// `finished` and gets no candidate: it stores nothing, but the kernel moves its state on as for id 0 (as the runtime's launch does
// for a finished row), so a row's states count up to its own end only.
extern "C" int wm_op_ts_states(int32_t* states, int32_t* picks, int32_t* out_tokens, int32_t* n_tokens, int32_t* pos, int32_t* ctl,
                               int32_t* key_lo, int32_t* tok_rows, int32_t* pos_rows, const int32_t* tokens, const int32_t* prompt_len,
                               const int32_t* n_ids, int B, int stride, int vocab, int timestamp_begin, int eos, int max_initial, int steps,
                               int row_prompts) {
    if (!states || !picks || !out_tokens || !n_tokens || !pos || !ctl || !tokens || !prompt_len || !n_ids || B <= 0 || B > (1 << 20) || stride <= 0 ||
        stride > (1 << 16) || vocab <= 0 || steps < 0)
        return fail(WM_E_ARG, "bad argument");
    WMCHK(ts_rules_check(vocab, timestamp_begin, eos));
    WMCHK(replay_rows_check(tokens, prompt_len, n_ids, B, stride, vocab));
    int Lmax = 0;
    for (int b = 0; b < B; ++b) Lmax = std::max(Lmax, prompt_len[b]);
    if (row_prompts) {
        if (!key_lo || !tok_rows || !pos_rows) return fail(WM_E_ARG, "row prompts need key_lo, tok_rows and pos_rows");
    } else {
        if (key_lo || tok_rows || pos_rows) return fail(WM_E_ARG, "key_lo, tok_rows and pos_rows belong to row prompts");
        if (prompt_len[0] > 16) return fail(WM_E_ARG, "the shared prompt holds at most 16 ids");
        for (int b = 1; b < B; ++b)
            if (prompt_len[b] != prompt_len[0] || !std::equal(tokens, tokens + prompt_len[0], tokens + (size_t)b * stride))
                return fail(WM_E_ARG, "row %d: the rows of a shared prompt start with the same ids", b);
    }
    const TsRules rules{timestamp_begin, eos, max_initial, vocab};
    TmpDev t;
    hipStream_t st = nullptr;
    DevBuf &out = t.add(), &nt = t.add(), &fin = t.add(), &dc = t.add(), &tr = t.add(), &pr = t.add(), &ts = t.add(), &kl = t.add(), &dpos = t.add(),
           &pv = t.add(), &pi = t.add(), &tv = t.add(), &ti = t.add(), &tm = t.add(), &tsum = t.add(), &nx = t.add(), &dlen = t.add();
    const size_t nb = (size_t)B * 4, no = (size_t)B * stride * 4, nr = (size_t)Lmax * B * 4;
    WMCHK(out.alloc(no, true));
    for (DevBuf* d : {&nt, &fin, &dpos, &pv, &pi, &tv, &ti, &tm, &tsum, &nx}) WMCHK(d->alloc(nb, true));
    WMCHK(dc.alloc(sizeof(StepCtl), true));
    WMCHK(ts.alloc((size_t)B * sizeof(TsState), true));
    if (row_prompts) {
        WMCHK(tr.alloc(nr, true));
        WMCHK(pr.alloc(nr, true));
        WMCHK(kl.alloc(nb, true));
        WMCHK(upload_bytes(dlen, prompt_len, nb));
    }
    InitDev d{out.as<int>(), nt.as<int>(), fin.as<int>(), row_prompts ? tr.as<int>() : nullptr, row_prompts ? pr.as<int>() : nullptr,
              row_prompts ? kl.as<int>() : nullptr, dc.as<StepCtl>(), ts.as<TsState>(), nullptr, nullptr};
    WMCHK(op_launch_init(t, d, tokens, prompt_len[0], row_prompts ? prompt_len : nullptr, stride, Lmax, B, stride, rules));
    if (row_prompts)
        launch_set_rows_step(dc.as<StepCtl>(), Lmax, dpos.as<int>(), dlen.as<int>(), 0, B, st);
    else
        launch_set_step(dc.as<StepCtl>(), Lmax, 1, dpos.as<int>(), Lmax, nullptr, 0, B, st);
    HIPCHK(hipGetLastError());
    const size_t sb = (size_t)B * sizeof(TsState);
    static_assert(sizeof(TsState) == 32, "a TsState is eight ints");
    HIPCHK(hipMemcpy(states, ts.p, sb, hipMemcpyDeviceToHost));
    const float ninf = -INFINITY;
    std::vector<int32_t> h_fin(B), h_pi(B), h_ti(B);
    std::vector<float> h_pv(B), h_tv(B), h_ts(B);
    for (int s = 1; s <= steps; ++s) {
        for (int b = 0; b < B; ++b) {
            const int at = prompt_len[b] + s - 1;
            h_fin[b] = at >= n_ids[b];
            const int id = h_fin[b] ? -1 : tokens[(size_t)b * stride + at];
            const bool text = id >= 0 && id < timestamp_begin, stamp = id >= timestamp_begin;
            h_pv[b] = text ? 0.f : ninf;
            h_pi[b] = text ? id : 0x7fffffff;
            h_tv[b] = stamp ? 0.f : ninf;  // the partial's value and its running maximum alike
            h_ti[b] = stamp ? id : 0x7fffffff;
            h_ts[b] = stamp ? 1.f : 0.f;
        }
        HIPCHK(hipMemcpy(fin.p, h_fin.data(), nb, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(pv.p, h_pv.data(), nb, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(pi.p, h_pi.data(), nb, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(tv.p, h_tv.data(), nb, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(tm.p, h_tv.data(), nb, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(ti.p, h_ti.data(), nb, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(tsum.p, h_ts.data(), nb, hipMemcpyHostToDevice));
        ArgmaxParams a{};
        a.V = vocab;
        a.B = B;
        a.pval = pv.as<float>();
        a.pidx = pi.as<int>();
        a.npart = 1;
        a.next = nx.as<int>();
        a.out_tokens = out.as<int>();
        a.out_stride = stride;
        a.n_tokens = nt.as<int>();
        a.finished = fin.as<int>();
        a.ctl = dc.as<StepCtl>();
        a.eot = -1;
        a.ignore_eot = 1;
        a.advance = 1;
        a.pos = dpos.as<int>();
        a.ts_state = ts.as<TsState>();
        a.rules = rules;
        a.ts_val = tv.as<float>();
        a.ts_idx = ti.as<int>();
        a.ts_m = tm.as<float>();
        a.ts_s = tsum.as<float>();
        a.ts_part0 = 0;
        LCHK(launch_argmax_step(a, st));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpy(states + (size_t)s * B * 8, ts.p, sb, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(picks + (size_t)(s - 1) * B, nx.p, nb, hipMemcpyDeviceToHost));
    }
    HIPCHK(hipMemcpy(out_tokens, out.p, no, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(n_tokens, nt.p, nb, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(pos, dpos.p, nb, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ctl, dc.p, sizeof(StepCtl), hipMemcpyDeviceToHost));
    if (row_prompts) {
        HIPCHK(hipMemcpy(key_lo, kl.p, nb, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(tok_rows, tr.p, nr, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(pos_rows, pr.p, nr, hipMemcpyDeviceToHost));
    }
    return 0;
}

// launch_set_rows_step alone: ctl [4] and pos [B_held] in and out, len [B].
extern "C" int wm_op_set_rows_step(int32_t* ctl, int32_t* pos, const int32_t* len, int Lmax, int pos_delta, int B, int B_held) {
    if (!ctl || !pos || !len || B <= 0 || B_held < B || B_held > (1 << 20)) return fail(WM_E_ARG, "bad argument");
    TmpDev t;
    DevBuf &dc = t.add(), &dp = t.add(), &dl = t.add();
    WMCHK(upload_bytes(dc, ctl, sizeof(StepCtl)));
    WMCHK(upload_bytes(dp, pos, (size_t)B_held * 4));
    WMCHK(upload_bytes(dl, len, (size_t)B * 4));
    launch_set_rows_step(dc.as<StepCtl>(), Lmax, dp.as<int>(), dl.as<int>(), pos_delta, B, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(ctl, dc.p, sizeof(StepCtl), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(pos, dp.p, (size_t)B_held * 4, hipMemcpyDeviceToHost));
    return 0;
}
// launch_set_step alone: ctl [4] in and out; pos, tok [B_held] in and out, each may be null (the kernel then leaves that side alone).
extern "C" int wm_op_set_step(int32_t* ctl, int32_t* pos, int32_t* tok, int len, int set_len, int pos_value, int tok_value, int B, int B_held) {
    if (!ctl || B <= 0 || B_held < B || B_held > (1 << 20)) return fail(WM_E_ARG, "bad argument");
    TmpDev t;
    DevBuf &dc = t.add(), &dp = t.add(), &dt = t.add();
    WMCHK(upload_bytes(dc, ctl, sizeof(StepCtl)));
    WMCHK(up_opt(dp, pos, (size_t)B_held * 4));
    WMCHK(up_opt(dt, tok, (size_t)B_held * 4));
    launch_set_step(dc.as<StepCtl>(), len, set_len, pos ? dp.as<int>() : nullptr, pos_value, tok ? dt.as<int>() : nullptr, tok_value, B, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(ctl, dc.p, sizeof(StepCtl), hipMemcpyDeviceToHost));
    WMCHK(down_opt(pos, dp, (size_t)B_held * 4));
    return down_opt(tok, dt, (size_t)B_held * 4);
}
// launch_pack_tokens alone: dst [rows_held][1 + stride] in and out (rows_held >= rows_cap >= rows), out_tokens [rows][out_stride],
// n_tokens [rows].  A row's min(n_tokens, stride) ids must lie inside its out_stride.
extern "C" int wm_op_pack_tokens(int32_t* dst, const int32_t* out_tokens, const int32_t* n_tokens, int out_stride, int rows, int rows_cap,
                                 int rows_held, int stride) {
    if (!dst || !out_tokens || !n_tokens || out_stride <= 0 || stride <= 0 || stride > (1 << 16) || out_stride > (1 << 16) || rows < 0 || rows_cap < rows ||
        rows_cap < 1 || rows_held < rows_cap || rows_held > (1 << 20))
        return fail(WM_E_ARG, "bad argument");
    for (int r = 0; r < rows; ++r)
        if (n_tokens[r] < 0 || std::min(n_tokens[r], stride) > out_stride) return fail(WM_E_ARG, "row %d: its ids reach past out_stride", r);
    TmpDev t;
    DevBuf &dd = t.add(), &dout = t.add(), &dn = t.add();
    WMCHK(upload_bytes(dd, dst, (size_t)rows_held * (1 + stride) * 4));
    WMCHK(upload_bytes(dout, out_tokens, (size_t)std::max(rows, 1) * out_stride * 4));
    WMCHK(upload_bytes(dn, n_tokens, (size_t)std::max(rows, 1) * 4));
    launch_pack_tokens(dout.as<int>(), dn.as<int>(), out_stride, rows, rows_cap, stride, dd.as<int>(), nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(dst, dd.p, (size_t)rows_held * (1 + stride) * 4, hipMemcpyDeviceToHost));
    return 0;
}
// launch_dec_embed alone: x [B_held][d] in and out, tok_emb [vocab][d], pos_emb [n_pos][d], tok / pos [B] inside their tables.
extern "C" int wm_op_dec_embed(float* x, const float* tok_emb, const float* pos_emb, const int32_t* tok, const int32_t* pos, int B, int B_held, int d,
                               int vocab, int n_pos) {
    if (!x || !tok_emb || !pos_emb || !tok || !pos || B <= 0 || B_held < B || B_held > (1 << 20) || d <= 0 || d > (1 << 14) || vocab <= 0 || n_pos <= 0)
        return fail(WM_E_ARG, "bad argument");
    for (int b = 0; b < B; ++b)
        if (tok[b] < 0 || tok[b] >= vocab || pos[b] < 0 || pos[b] >= n_pos) return fail(WM_E_ARG, "row %d: id or position outside its table", b);
    TmpDev t;
    DevBuf &dx = t.add(), &te = t.add(), &pe = t.add(), &dt = t.add(), &dp = t.add();
    WMCHK(upload_bytes(dx, x, (size_t)B_held * d * 4));
    WMCHK(upload_bytes(te, tok_emb, (size_t)vocab * d * 4));
    WMCHK(upload_bytes(pe, pos_emb, (size_t)n_pos * d * 4));
    WMCHK(upload_bytes(dt, tok, (size_t)B * 4));
    WMCHK(upload_bytes(dp, pos, (size_t)B * 4));
    launch_dec_embed(te.as<float>(), pe.as<float>(), dt.as<int>(), dp.as<int>(), dx.as<float>(), B, d, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(x, dx.p, (size_t)B_held * d * 4, hipMemcpyDeviceToHost));
    return 0;
}
// The two row copies: dst null — launch_no_speech_capture, rows [n_rows][d] -> out[0 .. n_rows); else launch_score_collect, rows[r] ->
// out[dst[r]] for dst[r] >= 0 (dst [n_rows] in [-1, out_rows)).  out [out_rows][d] in and out; d a multiple of 4 (16-byte copies).
extern "C" int wm_op_rows_copy(float* out, const float* rows, const int32_t* dst, int n_rows, int out_rows, int d) {
    if (!out || !rows || n_rows <= 0 || out_rows <= 0 || out_rows > (1 << 20) || n_rows > (1 << 20) || d <= 0 || d > (1 << 14) || d % 4)
        return fail(WM_E_ARG, "bad argument (d must be a multiple of 4)");
    if (!dst && out_rows < n_rows) return fail(WM_E_ARG, "the plain copy needs out_rows >= n_rows");
    if (dst)
        for (int r = 0; r < n_rows; ++r)
            if (dst[r] < -1 || dst[r] >= out_rows) return fail(WM_E_ARG, "dst[%d] = %d outside [-1, %d)", r, dst[r], out_rows);
    TmpDev t;
    DevBuf &o = t.add(), &in = t.add(), &dd = t.add();
    WMCHK(upload_bytes(o, out, (size_t)out_rows * d * 4));
    WMCHK(upload_bytes(in, rows, (size_t)n_rows * d * 4));
    if (dst) {
        WMCHK(upload_bytes(dd, dst, (size_t)n_rows * 4));
        launch_score_collect(in.as<float>(), o.as<float>(), dd.as<int>(), n_rows, d, nullptr);
    } else {
        launch_no_speech_capture(in.as<float>(), o.as<float>(), n_rows, d, nullptr);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, o.p, (size_t)out_rows * d * 4, hipMemcpyDeviceToHost));
    return 0;
}
// launch_mel_transpose_pad<T> alone on B clips: mel [B][C][L] fp32 -> image [B_held][L + 2][Cp] in dtype, Cp = C rounded up to 32, in
// (rounded to dtype on upload) and out (widened): the clips behind B are the guard.
extern "C" int wm_op_mel_transpose_pad(float* image, const float* mel, int B, int B_held, int C_in, int L, int dtype) {
    if (!image || !mel || B <= 0 || B_held < B || B_held > 64 || C_in <= 0 || C_in > 1024 || L <= 0 || L > (1 << 16)) return fail(WM_E_ARG, "bad argument");
    if (dtype < 0 || dtype > 2) return fail(WM_E_ARG, "bad dtype");
    const int Cp = (C_in + 31) / 32 * 32;
    const size_t n = (size_t)B_held * (L + 2) * Cp;
    TmpDev t;
    DevBuf &x = t.add(), &xt = t.add();
    WMCHK(upload(x, mel, (size_t)B * C_in * L, WM_F32));
    WMCHK(upload(xt, image, n, dtype));
    DISPATCH_DT(dtype, TT, launch_mel_transpose_pad<TT>(x.as<float>(), xt.p, B, C_in, L, Cp, nullptr));
    HIPCHK(hipGetLastError());
    return download_f32(image, xt, n, dtype);
}

// The no-speech probe's launches on the kernel variant wm_op_logits_lp would pick for (dtype, K, B): the LP sweep with
// no mask and no ranges, then no_speech_finish_kernel.  prob[b] = softmax(logits[b])[token], lse[b] = logsumexp(logits[b]).
extern "C" int wm_op_no_speech(float* prob, float* lse, const float* x, const float* ln_g, const float* ln_b, const float* emb, int B, int N, int K,
                               int dtype, int token) {
    if (!prob || !lse || !x || !ln_g || !ln_b || !emb || B <= 0 || N <= 0) return fail(WM_E_ARG, "bad argument");
    WMCHK(vocab_k_check(K));
    if (dtype < 0 || dtype > 2) return fail(WM_E_ARG, "bad dtype");
    if (token < 0 || token >= N) return fail(WM_E_ARG, "token %d is not a vocabulary id", token);
    TmpDev t;
    const int npart = dec_logits_parts(N);
    const float* dx;
    VocabHead vh;
    WMCHK(upload_vocab_head(t, x, ln_g, ln_b, emb, B, N, K, dtype, &dx, &vh));
    DevBuf &pm = t.add(), &pi = t.add(), &ps = t.add(), &pr = t.add(), &ls = t.add();
    for (DevBuf* d : {&pm, &pi, &ps}) WMCHK(d->alloc((size_t)B * npart * 4, true));
    WMCHK(pr.alloc((size_t)B * 4, true));
    WMCHK(ls.alloc((size_t)B * 4, true));
    WMCHK(ns_sweep(dtype, dx, vh, B, npart, pm.as<float>(), pi.as<int>(), ps.as<float>(), token, pr.as<float>(), ls.as<float>(), nullptr));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(prob, pr.p, (size_t)B * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(lse, ls.p, (size_t)B * 4, hipMemcpyDeviceToHost));
    return 0;
}

// lang_detect_kernel alone, launched as the language pass launches it (no patch).
extern "C" int wm_op_lang_detect(int32_t* lang_out, float* probs, const float* x, const float* ln_g, const float* ln_b, const float* emb,
                                 const int32_t* lang_ids, int n_lang, int B, int N, int K, int dtype) {
    if (!lang_out || !x || !ln_g || !ln_b || !emb || !lang_ids || B <= 0 || N <= 0) return fail(WM_E_ARG, "bad argument");
    WMCHK(vocab_k_check(K));
    if (dtype < 0 || dtype > 2) return fail(WM_E_ARG, "bad dtype");
    WMCHK(lang_list_check(N, lang_ids, n_lang));
    TmpDev t;
    const float* dx;
    VocabHead vh;
    WMCHK(upload_vocab_head(t, x, ln_g, ln_b, emb, B, N, K, dtype, &dx, &vh));
    DevBuf &li = t.add(), &lo = t.add(), &pr = t.add();
    WMCHK(upload_bytes(li, lang_ids, (size_t)n_lang * 4));
    WMCHK(lo.alloc((size_t)B * 4, true));
    WMCHK(pr.alloc((size_t)B * n_lang * 4, true));
    LangDetectParams q{};
    q.x = dx;
    q.ldx = K;
    q.ln_g = vh.ln_g;
    q.ln_b = vh.ln_b;
    q.emb = vh.emb;
    q.lang_ids = li.as<int>();
    q.n_lang = n_lang;
    q.K = K;
    q.B = B;
    q.lang_out = lo.as<int>();
    q.probs = pr.as<float>();
    DISPATCH_DT(dtype, TT, launch_lang_detect<TT>(q, nullptr));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(lang_out, lo.p, (size_t)B * 4, hipMemcpyDeviceToHost));
    if (probs) HIPCHK(hipMemcpy(probs, pr.p, (size_t)B * n_lang * 4, hipMemcpyDeviceToHost));
    return 0;
}

// The absorbed cross-attention of m->xattn models, wired as launch_cross_attn + cross_attn_merge wire it: absorb, X sweep, merge.
static int op_xattn(float* out, const float* q, const float* Wk, const float* Wv, const float* bv, const float* X, int rows, int q_B, int n_utt,
                    int n_keys, int n_heads, int nsplit, int out_dtype, const int32_t* utt_of);
extern "C" int wm_op_xattn(float* out, const float* q, const float* Wk, const float* Wv, const float* bv, const float* X, int rows,
                           int q_B, int n_utt, int n_keys, int n_heads, int nsplit, int out_dtype) {
    return op_xattn(out, q, Wk, Wv, bv, X, rows, q_B, n_utt, n_keys, n_heads, nsplit, out_dtype, nullptr);
}
// X by row map: X holds n_utt clips, the row in batch slot b (of q_B slots, or of `rows` when q_B == 0) sweeps clip utt_of[b]
extern "C" int wm_op_xattn_map(float* out, const float* q, const float* Wk, const float* Wv, const float* bv, const float* X, int rows,
                               int q_B, int n_utt, int n_keys, int n_heads, int nsplit, int out_dtype, const int32_t* utt_of) {
    if (!utt_of) return fail(WM_E_ARG, "bad argument");
    return op_xattn(out, q, Wk, Wv, bv, X, rows, q_B, n_utt, n_keys, n_heads, nsplit, out_dtype, utt_of);
}
static int op_xattn(float* out, const float* q, const float* Wk, const float* Wv, const float* bv, const float* X, int rows, int q_B, int n_utt,
                    int n_keys, int n_heads, int nsplit, int out_dtype, const int32_t* utt_of) {
    if (!out || !q || !Wk || !Wv || !bv || !X || rows <= 0 || n_utt <= 0 || n_keys <= 0) return fail(WM_E_ARG, "bad argument");
    if (n_heads < 1 || n_heads > 8 || nsplit < 1 || nsplit > 64) return fail(WM_E_ARG, "needs 1 <= n_heads <= 8, 1 <= nsplit <= 64");
    if (out_dtype != WM_F32 && out_dtype != WM_BF16) return fail(WM_E_ARG, "out_dtype must be WM_F32 or WM_BF16");
    if (utt_of) {  // any number of rows per clip: the map alone says which
        if (q_B < 0 || (q_B > 0 && rows % q_B)) return fail(WM_E_ARG, "rows must be P * q_B (prefill)");
        for (int b = 0, n = q_B > 0 ? q_B : rows; b < n; ++b)
            if (utt_of[b] < 0 || utt_of[b] >= n_utt) return fail(WM_E_ARG, "utt_of[%d] = %d outside [0, %d)", b, utt_of[b], n_utt);
    } else if (q_B < 0 || (q_B > 0 ? (q_B > n_utt || rows % q_B) : rows > n_utt))
        return fail(WM_E_ARG, "rows must be P * q_B with q_B <= n_utt (prefill), or <= n_utt (q_B == 0)");
    const size_t d = (size_t)n_heads * 64;
    TmpDev t;
    hipStream_t st = nullptr;
    DevBuf &dq = t.add(), &wk = t.add(), &wv = t.add(), &b = t.add(), &dx = t.add(), &qs = t.add(), &py = t.add(), &pml = t.add(),
           &o = t.add();
    WMCHK(upload(dq, q, (size_t)rows * d, WM_F32));
    WMCHK(upload(wk, Wk, d * d, WM_BF16));
    WMCHK(upload(wv, Wv, d * d, WM_BF16));
    WMCHK(upload(b, bv, d, WM_F32));
    WMCHK(upload(dx, X, (size_t)n_utt * n_keys * d, WM_BF16));
    WMCHK(qs.alloc((size_t)rows * 3 * n_heads * d * 2, true));
    WMCHK(py.alloc((size_t)rows * nsplit * n_heads * d * 4, true));
    WMCHK(pml.alloc((size_t)rows * nsplit * n_heads * 2 * 4, true));
    WMCHK(o.alloc((size_t)rows * d * dt_size(out_dtype), true));
    DevBuf& dmap = t.add();
    if (utt_of) WMCHK(upload_bytes(dmap, utt_of, (size_t)(q_B > 0 ? q_B : rows) * 4));
    XAttnParams x{};
    x.q = dq.as<float>();
    x.Wk = wk.p;
    x.Wv = wv.p;
    x.bv = b.as<float>();
    x.X = dx.p;
    x.x_stride = (long)((size_t)n_keys * d);
    x.n_keys = n_keys;
    x.nsplit = nsplit;
    x.H = n_heads;
    x.d = (int)d;
    x.rows = rows;
    x.q_B = q_B;
    x.scale = ATTN_SCALE;
    x.qs = qs.p;
    x.part_y = py.as<float>();
    x.part_ml = pml.as<float>();
    x.out = o.p;
    x.out_dtype = out_dtype;
    LCHK(launch_xattn_absorb(x, st));
    LCHK(launch_xattn(x, st, utt_of ? dmap.as<int>() : nullptr));
    LCHK(launch_xattn_merge(x, st));
    HIPCHK(hipGetLastError());
    return download_f32(out, o, (size_t)rows * d, out_dtype);
}

// xattn_absorb_kernel alone: the three bf16 images of q' as the X sweep reads them
extern "C" int wm_op_xattn_absorb(float* images, const float* q, const float* Wk, int rows, int n_heads, int late_loads) {
    if (!images || !q || !Wk || rows <= 0) return fail(WM_E_ARG, "bad argument");
    if (n_heads < 1 || n_heads > 8) return fail(WM_E_ARG, "needs 1 <= n_heads <= 8");
    const size_t d = (size_t)n_heads * 64, n = (size_t)rows * 3 * n_heads * d;
    TmpDev t;
    DevBuf &dq = t.add(), &wk = t.add(), &qs = t.add();
    WMCHK(upload(dq, q, (size_t)rows * d, WM_F32));
    WMCHK(upload(wk, Wk, d * d, WM_BF16));
    WMCHK(qs.alloc(n * 2, true));
    XAttnParams x{};
    x.q = dq.as<float>();
    x.Wk = wk.p;
    x.n_keys = 1;  // (not read by the absorb; the launch check wants a key)
    x.nsplit = 1;
    x.H = n_heads;
    x.d = (int)d;
    x.rows = rows;
    x.scale = ATTN_SCALE;
    x.qs = qs.p;
    LCHK(launch_xattn_absorb(x, nullptr, late_loads != 0));
    HIPCHK(hipGetLastError());
    return download_f32(images, qs, n, WM_BF16);
}

extern "C" int wm_op_gelu(float* tt, size_t n, int mode) {
    if (!tt || (mode != 0 && mode != 1)) return fail(WM_E_ARG, "bad argument");
    if (n == 0) return 0;
    TmpDev t;
    DevBuf& x = t.add();
    WMCHK(upload(x, tt, n, WM_F32));
    launch_gelu(x.as<float>(), n, mode, nullptr);
    HIPCHK(hipMemcpy(tt, x.p, n * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int wm_op_softmax_rows(float* tt, int rows, int cols) {
    if (!tt || rows <= 0 || cols <= 0) return fail(WM_E_ARG, "bad argument");
    TmpDev t;
    DevBuf& x = t.add();
    WMCHK(upload(x, tt, (size_t)rows * cols, WM_F32));
    launch_softmax_rows(x.as<float>(), rows, cols, nullptr);
    HIPCHK(hipMemcpy(tt, x.p, (size_t)rows * cols * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int wm_op_argmax(const float* tt, int n, int32_t* idx) {
    if (!tt || !idx || n <= 0) return fail(WM_E_ARG, "bad argument");
    TmpDev t;
    DevBuf &x = t.add(), &o = t.add();
    WMCHK(upload(x, tt, n, WM_F32));
    WMCHK(o.alloc(4));
    launch_argmax_plain(x.as<float>(), n, o.as<int>(), nullptr);
    HIPCHK(hipMemcpy(idx, o.p, 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int wm_op_conv1d_k3(float* out, const float* inp, const float* weight, const float* bias, int C_in, int L_in,
                               int C_out, int stride, int out_T, int dtype) {
    if (!out || !inp || !weight || !bias || C_in <= 0 || L_in <= 0 || C_out <= 0) return fail(WM_E_ARG, "bad argument");
    if (stride != 1 && stride != 2) return fail(WM_E_ARG, "stride must be 1 or 2");
    if (C_out % 128) return fail(WM_E_ARG, "C_out must be a multiple of 128");
    if (dtype < 0 || dtype > 2) return fail(WM_E_ARG, "bad dtype");
    const int Cp = (C_in + 31) / 32 * 32;
    const int L_out = (L_in + 2 - 3) / stride + 1;
    TmpDev t;
    DevBuf &x = t.add(), &xt = t.add(), &w = t.add(), &b = t.add(), &o = t.add(), &o2 = t.add();
    WMCHK(upload(x, inp, (size_t)C_in * L_in, WM_F32));
    WMCHK(xt.alloc(((size_t)L_in + 2 + 512) * Cp * dt_size(dtype), true));
    auto wr = conv_relayout(weight, C_out, C_in, Cp);
    WMCHK(upload(w, wr.data(), wr.size(), dtype));
    WMCHK(upload(b, bias, C_out, WM_F32));
    WMCHK(o.alloc((size_t)L_out * C_out * 4));
    DISPATCH_DT(dtype, TT, launch_mel_transpose_pad<TT>(x.as<float>(), xt.p, 1, C_in, L_in, Cp, nullptr));
    GemmParams p{};
    p.A = xt.p;
    p.W = w.p;
    p.C = o.p;
    p.M = L_out;
    p.N = C_out;
    p.K = 3 * Cp;
    p.lda = (long)stride * Cp;
    p.ldw = 3 * Cp;
    p.ldc = C_out;
    p.bias = b.as<float>();
    WMCHK(gemm_dispatch(dtype, WM_F32, p, 1, nullptr));
    if (out_T) {
        HIPCHK(hipMemcpy(out, o.p, (size_t)L_out * C_out * 4, hipMemcpyDeviceToHost));
    } else {
        WMCHK(o2.alloc((size_t)L_out * C_out * 4));
        launch_transpose_f32(o.as<float>(), o2.as<float>(), L_out, C_out, nullptr);
        HIPCHK(hipMemcpy(out, o2.p, (size_t)L_out * C_out * 4, hipMemcpyDeviceToHost));
    }
    HIPCHK(hipGetLastError());
    return 0;
}
