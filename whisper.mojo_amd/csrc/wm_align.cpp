// wm_align.cpp — the alignment chain: the alignment heads, the buffers and parameters of a timestamp or align pass, the
// post-loop kernels behind a pass, and the chain's wm_op_* hooks, which use its helpers.
#include "wm_runtime.h"

// ---- token-level timestamps ------------------------------------------------------------------------------------
extern "C" int wm_set_alignment_heads(wm_model* m, const int32_t* layer_head_pairs, int n_pairs) {
    if (!m || n_pairs < 0 || (n_pairs > 0 && !layer_head_pairs)) return fail(WM_E_ARG, "bad argument");
    if (n_pairs > ALIGN_MAX_HEADS) return fail(WM_E_ARG, "at most %d alignment heads (got %d)", ALIGN_MAX_HEADS, n_pairs);
    const wm_dims& c = m->cfg.dims;
    std::vector<int32_t> pairs(layer_head_pairs, layer_head_pairs + 2 * n_pairs);
    for (int k = 0; k < n_pairs; ++k) {
        const int l = pairs[2 * k], h = pairs[2 * k + 1];
        if (l < 0 || l >= c.n_layers || h < 0 || h >= c.n_heads || h >= 32)
            return fail(WM_E_ARG, "alignment head %d = (%d, %d) outside %d layers x %d heads", k, l, h, c.n_layers, c.n_heads);
        for (int q = 0; q < k; ++q)
            if (pairs[2 * q] == l && pairs[2 * q + 1] == h) return fail(WM_E_ARG, "alignment head (%d, %d) listed twice", l, h);
    }
    m->align_pairs = pairs;
    return 0;
}

// The buffers of a timestamp or align pass (they only grow) for al.pairs: Lr >= 1 rows per utterance, times_stride time columns
int align_buffers(wm_model* m, wm_state* s, size_t Lr, size_t times_stride) {
    wm_state::Align& a = s->al;
    const size_t B = s->B, T = m->cfg.dims.n_audio_ctx, n_sel = a.pairs.size() / 2;
    WMCHK(grow(a.cap, B * Lr * n_sel * 64 * 4));
    if (m->xattn) WMCHK(grow(a.kh, B * n_sel * T * 64 * 4));
    WMCHK(grow(a.probs, B * n_sel * Lr * T * 4));
    WMCHK(grow(a.mean, B * n_sel * T * 4));
    WMCHK(grow(a.stdv, B * n_sel * T * 4));
    WMCHK(grow(a.M, B * Lr * T * 4));
    // rows past ~400 at n_audio_ctx = 1500: the 2-bit trace leaves LDS for global memory
    if (align_dtw_lds_bytes((int)Lr, (int)T) == 0) WMCHK(grow(a.trace, B * Lr * ((T + 15) / 16) * 4));
    WMCHK(grow(a.times, B * times_stride * 4));
    WMCHK(grow(a.ncols, B * 4));
    return 0;
}
// Before the pass's graphs are (re)captured: size the timestamp buffers of state s and record what the pass asked for.
int align_setup(wm_model* m, wm_state* s, const wm_decode_opts* o, const std::vector<int32_t>* cols, const WinAsk* win) {
    wm_state::Align& a = s->al;
    a.on = cols != nullptr;
    a.win = a.on && win != nullptr;
    if (!a.on) return 0;
    if (a.win) {  // the tables the window kernel fills, and what it hands back
        a.items = win->items;
        a.n_real = win->n_real;
        WMCHK(grow(a.rows, (size_t)s->B * 4));
        WMCHK(grow(a.row0, (size_t)s->B * 4));
        WMCHK(grow(a.wtimes, (size_t)s->B * (o->max_loop + 1) * 8));
    }
    a.pairs = m->align_pairs;
    a.L = o->max_loop;
    a.n_prompt = o->n_prompt;
    a.cols = *cols;
    ++a.gen;
    WMCHK(align_buffers(m, s, std::max<size_t>(o->max_loop, 1), s->out_stride));
    // (a.cols outlives the copy: the state is not reused before this pass is waited for)
    HIPCHK(hipMemcpyAsync(a.ncols.p, a.cols.data(), (size_t)s->B * 4, hipMemcpyHostToDevice, s->lanes[0].st));
    return 0;
}

static AlignParams align_params(wm_model* m, wm_state* s) {
    const wm_dims& c = m->cfg.dims;
    const wm_state::Align& a = s->al;
    AlignParams p{};
    p.cap = a.cap.as<float>();
    p.B = s->B;
    p.L = a.L;
    p.n_sel = (int)a.pairs.size() / 2;
    p.n_prompt = a.n_prompt;
    p.T = c.n_audio_ctx;
    p.d = c.d_model;
    p.n_tokens = s->n_tokens.as<int>();
    p.n_frames = a.ncols.as<int>();
    if (m->xattn) {
        p.X = s->enc_x.p;
        p.Wk = m->cross_kv_w.p;
        p.kh = a.kh.as<float>();
    } else {
        p.kv = s->cross_kv.p;
        p.kv_dtype = m->cfg.kv_dtype;
        p.kv_layer_stride = (long)((size_t)s->B * c.n_audio_ctx * c.d_model);
    }
    for (int k = 0; k < p.n_sel; ++k) {
        p.layer[k] = a.pairs[2 * k];
        p.head[k] = a.pairs[2 * k + 1];
    }
    p.probs = a.probs.as<float>();
    p.mean = a.mean.as<float>();
    p.stdv = a.stdv.as<float>();
    p.M = a.M.as<float>();
    p.trace = align_dtw_lds_bytes(a.L, c.n_audio_ctx) ? nullptr : a.trace.as<unsigned>();
    p.times = a.times.as<float>();
    p.out_stride = s->out_stride;
    if (a.ragged) {  // an align pass: per-row row counts and offsets, the caller's table width
        p.n_tokens = nullptr;
        p.n_prompt = 0;
        p.rows = a.rows.as<int>();
        p.row0 = a.row0.as<int>();
        p.out_stride = a.stride;
        for (int b = 0; b < s->B; ++b) p.out_need = std::max(p.out_need, a.h_row0[b] + a.h_rows[b] + 1);
    } else if (a.win) {  // a window pass: the same form, the tables made on the device (row0[b] <= n_prompt, rows[b] <= L)
        p.n_tokens = nullptr;
        p.rows = a.rows.as<int>();
        p.row0 = a.row0.as<int>();
        p.out_need = a.n_prompt + a.L + 1;
    }
    return p;
}
static AlignWindowParams align_window_params(wm_state* s, int mode) {
    const wm_state::Align& a = s->al;
    AlignWindowParams w{};
    w.mode = mode;
    w.B = s->B;
    w.n_real = a.n_real;
    w.L = a.L;
    w.n_prompt = a.n_prompt;
    w.out_stride = s->out_stride;
    w.n_tokens = s->n_tokens.as<int>();
    w.prompt_len = s->rw.on ? s->rw.len.as<int>() : nullptr;
    w.items = a.items;
    w.rows = a.rows.as<int>();
    w.row0 = a.row0.as<int>();
    w.times = a.times.as<float>();
    w.out = (double*)a.wtimes.p;
    return w;
}

// the post-loop kernels of a timestamp pass, on lane 0's stream behind the last step
int enqueue_align(wm_model* m, wm_state* s) {
    hipStream_t st = s->lanes[0].st;
    if (s->al.L == 0) {  // max_loop 0: no row ever, every time is 0 (HF's early return)
        HIPCHK(hipMemsetAsync(s->al.times.p, 0, (size_t)s->B * (s->al.ragged ? s->al.stride : s->out_stride) * 4, st));
        if (s->al.win) LCHK(launch_align_window(align_window_params(s, 1), st));  // the one id of each window, at its offset
        return 0;
    }
    const AlignParams p = align_params(m, s);
    if (s->al.win) LCHK(launch_align_window(align_window_params(s, 0), st));  // rows / row0 from the loop's counts
    LCHK(launch_align_probs(p, st));
    LCHK(launch_align_norm(p, st));
    LCHK(launch_align_dtw(p, st));
    if (s->al.win) LCHK(launch_align_window(align_window_params(s, 1), st));  // the window's result rows
    return 0;
}

extern "C" int wm_alignment_weights(wm_model* m, int slot, float* out) {
    if (!m || !out || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument");
    const wm_model::AlignRef& r = m->align_ref[slot];
    if (!r.st || !state_is_live(r.st) || r.st->al.gen != r.gen || r.st->pending)
        return fail(WM_E_STATE, "no completed timestamp pass on this slot (or its state has run another pass since)");
    wm_state* s = r.st;
    const size_t T = m->cfg.dims.n_audio_ctx, L = s->al.L, n_sel = s->al.pairs.size() / 2;
    HIPCHK(hipSetDevice(m->device));
    const size_t per_row = n_sel * L * T;
    HIPCHK(hipMemcpy(out, s->al.probs.as<float>() + (size_t)r.row0 * per_row, (size_t)r.rows * per_row * 4, hipMemcpyDeviceToHost));
    std::vector<int32_t> n(r.rows);
    HIPCHK(hipMemcpy(n.data(), s->n_tokens.as<int>() + r.row0, (size_t)r.rows * 4, hipMemcpyDeviceToHost));
    for (int b = 0; b < r.rows; ++b) {  // rows past R_b were never computed
        const size_t R = s->al.ragged ? (size_t)s->al.h_rows[r.row0 + b] : (size_t)std::max(0, std::min<int>((int)L, n[b] - s->al.n_prompt - 1));
        for (size_t k = 0; k < n_sel; ++k) std::fill(out + b * per_row + (k * L + R) * T, out + b * per_row + (k + 1) * L * T, 0.f);
    }
    return 0;
}

extern "C" int wm_op_token_times(float* times, const float* weights, int n_sel, int R, int F, int n_prompt) {
    if (!times || n_sel <= 0 || n_sel > ALIGN_MAX_HEADS || R < 0 || R > ALIGN_MAX_ROWS || F <= 0 || n_prompt < 0 || (R > 0 && !weights))
        return fail(WM_E_ARG, "bad argument (1 <= n_sel <= %d, 0 <= R <= %d, F >= 1)", ALIGN_MAX_HEADS, ALIGN_MAX_ROWS);
    const int total = n_prompt + R + 1;
    if (R == 0) {
        std::fill(times, times + total, 0.f);
        return 0;
    }
    TmpDev t;
    DevBuf &probs = t.add(), &mean = t.add(), &sd = t.add(), &M = t.add(), &tr = t.add(), &tm = t.add(), &nt = t.add();
    WMCHK(upload(probs, weights, (size_t)n_sel * R * F, WM_F32));
    WMCHK(mean.alloc((size_t)n_sel * F * 4));
    WMCHK(sd.alloc((size_t)n_sel * F * 4));
    WMCHK(M.alloc((size_t)R * F * 4));
    WMCHK(tm.alloc((size_t)total * 4));
    WMCHK(upload_bytes(nt, &total, 4));
    AlignParams p{};
    p.B = 1;
    p.L = R;
    p.n_sel = n_sel;
    p.n_prompt = n_prompt;
    p.T = F;
    p.n_tokens = nt.as<int>();
    p.probs = probs.as<float>();
    p.mean = mean.as<float>();
    p.stdv = sd.as<float>();
    p.M = M.as<float>();
    if (align_dtw_lds_bytes(R, F) == 0) {
        WMCHK(tr.alloc((size_t)R * ((F + 15) / 16) * 4));
        p.trace = tr.as<unsigned>();
    }
    p.times = tm.as<float>();
    p.out_stride = total;
    LCHK(launch_align_norm(p, nullptr));
    LCHK(launch_align_dtw(p, nullptr));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(times, tm.p, (size_t)total * 4, hipMemcpyDeviceToHost));
    return 0;
}

// Several weight tables through align_norm and align_dtw in ONE launch each, with per-table row counts and offsets (the ragged chain of
// an align pass): weights [n_tab][n_sel][L][T] with L >= max R and T >= max F, table b's R[b] x F[b] corner used;
// times [n_tab][out_stride], out_stride >= max(row0[b] + R[b] + 1).
extern "C" int wm_op_token_times_rows(float* times, const float* weights, int n_tab, int n_sel, int L, int T, const int32_t* R, const int32_t* F,
                                      const int32_t* row0, int out_stride) {
    if (!times || !weights || !R || !F || !row0 || n_tab <= 0 || n_sel <= 0 || n_sel > ALIGN_MAX_HEADS || L <= 0 || L > ALIGN_MAX_ROWS || T <= 0)
        return fail(WM_E_ARG, "bad argument (1 <= n_sel <= %d, 1 <= L <= %d, T >= 1)", ALIGN_MAX_HEADS, ALIGN_MAX_ROWS);
    int need = 0;
    for (int b = 0; b < n_tab; ++b) {
        if (R[b] < 0 || R[b] > L || F[b] < 1 || F[b] > T || row0[b] < 0) return fail(WM_E_ARG, "table %d: R in [0, L], F in [1, T], row0 >= 0", b);
        need = std::max(need, row0[b] + R[b] + 1);
    }
    if (out_stride < need) return fail(WM_E_ARG, "out_stride %d is smaller than max(row0 + R + 1) = %d", out_stride, need);
    TmpDev t;
    DevBuf &probs = t.add(), &mean = t.add(), &sd = t.add(), &M = t.add(), &tr = t.add(), &tm = t.add(), &dr = t.add(), &df = t.add(), &d0 = t.add();
    WMCHK(upload(probs, weights, (size_t)n_tab * n_sel * L * T, WM_F32));
    WMCHK(mean.alloc((size_t)n_tab * n_sel * T * 4));
    WMCHK(sd.alloc((size_t)n_tab * n_sel * T * 4));
    WMCHK(M.alloc((size_t)n_tab * L * T * 4));
    WMCHK(tm.alloc((size_t)n_tab * out_stride * 4));
    for (auto pr : {std::make_pair(&dr, R), std::make_pair(&df, F), std::make_pair(&d0, row0)}) WMCHK(upload_bytes(*pr.first, pr.second, (size_t)n_tab * 4));
    AlignParams p{};
    p.B = n_tab;
    p.L = L;
    p.n_sel = n_sel;
    p.T = T;
    p.n_frames = df.as<int>();
    p.rows = dr.as<int>();
    p.row0 = d0.as<int>();
    p.out_need = need;
    p.probs = probs.as<float>();
    p.mean = mean.as<float>();
    p.stdv = sd.as<float>();
    p.M = M.as<float>();
    if (align_dtw_lds_bytes(L, T) == 0) {
        WMCHK(tr.alloc((size_t)n_tab * L * ((T + 15) / 16) * 4));
        p.trace = tr.as<unsigned>();
    }
    p.times = tm.as<float>();
    p.out_stride = out_stride;
    LCHK(launch_align_norm(p, nullptr));
    LCHK(launch_align_dtw(p, nullptr));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(times, tm.p, (size_t)n_tab * out_stride * 4, hipMemcpyDeviceToHost));
    return 0;
}

// launch_align_probs alone.  Keys: kv (host fp32 [n_layers][2][B][T][d], the model's K/V cache with its V halves, uploaded as
// kv_dtype) or the absorbed form X [B][T][d] + Wk [n_layers][2][d][d] (both uploaded as bf16, K_h built in a scratch buffer).
// probs [B][n_sel][L][T] goes up before the launch and comes back after it: rows >= rows[b] keep what the caller put there.
extern "C" int wm_op_align_probs(float* probs, const float* q, const float* kv, int kv_dtype, const float* X, const float* Wk,
                                 const int32_t* layer_head_pairs, int n_sel, const int32_t* rows, int B, int L, int T, int d, int n_layers) {
    if (!probs || !q || !layer_head_pairs || !rows) return fail(WM_E_ARG, "probs, q, layer_head_pairs and rows are required");
    if (kv ? (X || Wk) : (!X || !Wk)) return fail(WM_E_ARG, "keys: either kv, or X and Wk");
    if (kv && kv_dtype != WM_F32 && kv_dtype != WM_BF16 && kv_dtype != WM_F16) return fail(WM_E_ARG, "kv_dtype %d", kv_dtype);
    if (B <= 0 || n_sel <= 0 || n_sel > ALIGN_MAX_HEADS || L <= 0 || L > ALIGN_MAX_ROWS || T <= 0 || d <= 0 || d % 64 || n_layers <= 0)
        return fail(WM_E_ARG, "bad argument (B >= 1, 1 <= n_sel <= %d, 1 <= L <= %d, T >= 1, d a multiple of 64, n_layers >= 1)", ALIGN_MAX_HEADS,
                    ALIGN_MAX_ROWS);
    for (int b = 0; b < B; ++b)
        if (rows[b] < 0 || rows[b] > L) return fail(WM_E_ARG, "utterance %d: rows in [0, L]", b);
    for (int k = 0; k < n_sel; ++k)
        if (layer_head_pairs[2 * k] < 0 || layer_head_pairs[2 * k] >= n_layers || layer_head_pairs[2 * k + 1] < 0 || layer_head_pairs[2 * k + 1] >= d / 64)
            return fail(WM_E_ARG, "pair %d: layer in [0, %d), head in [0, %d)", k, n_layers, d / 64);
    TmpDev t;
    DevBuf &cap = t.add(), &keys = t.add(), &wk = t.add(), &kh = t.add(), &pr = t.add(), &dr = t.add();
    WMCHK(upload(cap, q, (size_t)B * L * n_sel * 64, WM_F32));
    WMCHK(upload(pr, probs, (size_t)B * n_sel * L * T, WM_F32));
    WMCHK(upload_bytes(dr, rows, (size_t)B * 4));
    AlignParams p{};
    p.cap = cap.as<float>();
    p.B = B;
    p.L = L;
    p.n_sel = n_sel;
    p.T = T;
    p.d = d;
    p.rows = dr.as<int>();
    if (kv) {
        WMCHK(upload(keys, kv, (size_t)n_layers * 2 * B * T * d, kv_dtype));
        p.kv = keys.p;
        p.kv_dtype = kv_dtype;
        p.kv_layer_stride = (long)((size_t)B * T * d);
    } else {
        WMCHK(upload(keys, X, (size_t)B * T * d, WM_BF16));
        WMCHK(upload(wk, Wk, (size_t)n_layers * 2 * d * d, WM_BF16));
        WMCHK(kh.alloc((size_t)B * n_sel * T * 64 * 4));
        p.X = keys.p;
        p.Wk = wk.p;
        p.kh = kh.as<float>();
    }
    for (int k = 0; k < n_sel; ++k) {
        p.layer[k] = layer_head_pairs[2 * k];
        p.head[k] = layer_head_pairs[2 * k + 1];
    }
    p.probs = pr.as<float>();
    LCHK(launch_align_probs(p, nullptr));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(probs, pr.p, (size_t)B * n_sel * L * T * 4, hipMemcpyDeviceToHost));
    return 0;
}

// launch_align_norm alone: wm_op_token_times_rows' tables -> M [n_tab][L][T], uploaded first (cells outside a table's R x F corner keep
// what the caller put there).
extern "C" int wm_op_align_norm(float* M, const float* weights, int n_tab, int n_sel, int L, int T, const int32_t* R, const int32_t* F) {
    if (!M || !weights || !R || !F || n_tab <= 0 || n_sel <= 0 || n_sel > ALIGN_MAX_HEADS || L <= 0 || L > ALIGN_MAX_ROWS || T <= 0)
        return fail(WM_E_ARG, "bad argument (1 <= n_sel <= %d, 1 <= L <= %d, T >= 1)", ALIGN_MAX_HEADS, ALIGN_MAX_ROWS);
    for (int b = 0; b < n_tab; ++b)
        if (R[b] < 0 || R[b] > L || F[b] < 1 || F[b] > T) return fail(WM_E_ARG, "table %d: R in [0, L], F in [1, T]", b);
    TmpDev t;
    DevBuf &probs = t.add(), &mean = t.add(), &sd = t.add(), &dm = t.add(), &dr = t.add(), &df = t.add();
    WMCHK(upload(probs, weights, (size_t)n_tab * n_sel * L * T, WM_F32));
    WMCHK(upload(dm, M, (size_t)n_tab * L * T, WM_F32));
    WMCHK(mean.alloc((size_t)n_tab * n_sel * T * 4));
    WMCHK(sd.alloc((size_t)n_tab * n_sel * T * 4));
    for (auto pr : {std::make_pair(&dr, R), std::make_pair(&df, F)}) WMCHK(upload_bytes(*pr.first, pr.second, (size_t)n_tab * 4));
    AlignParams p{};
    p.B = n_tab;
    p.L = L;
    p.n_sel = n_sel;
    p.T = T;
    p.n_frames = df.as<int>();
    p.rows = dr.as<int>();
    p.probs = probs.as<float>();
    p.mean = mean.as<float>();
    p.stdv = sd.as<float>();
    p.M = dm.as<float>();
    LCHK(launch_align_norm(p, nullptr));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(M, dm.p, (size_t)n_tab * L * T * 4, hipMemcpyDeviceToHost));
    return 0;
}
