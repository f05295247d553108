// wm_bench.cpp — the measurement helpers behind bench.py and tools/: wm_bench_bytes and wm_bench_kernel.
#include <cstdio>

#include "wm_runtime.h"
// ---- measurement helpers ------------------------------------------------------------------------------------------------
// A freshly encoded state has an empty self-attention cache; the decode step is priced AND timed mid-sequence, at this many
// cached rows (SURVEY §8d quotes its byte figures at t = 50; the rows of a fresh cache are zero, which the timing does not care about)
static const int BENCH_STEP_LEN = 50;
extern "C" int wm_bench_bytes(wm_model* m, wm_state* s, int which, double* bytes) {
    if (!m || !s || !bytes) return fail(WM_E_ARG, "null argument");
    if (!state_is_live(s) || s->m != m) return fail(WM_E_ARG, "stale or foreign state handle");
    const wm_dims& c = m->cfg.dims;
    const double d = c.d_model, H = c.n_heads, B = s->B;
    const double ks = dt_size(m->cfg.kv_dtype), ws = dt_size(dec_dtype(m->cfg));
    // m->xattn: the cross-attention of one layer (absorb + sweep + merge, as wm_bench_kernel times it) reads X (bf16) once per
    // utterance, Wk and Wv (bf16) once, q' (three bf16 images) per row (written and read), and writes / re-reads H·d partials per key chunk
    const double x_layer = B * (double)c.n_audio_ctx * d * 2 + 2 * d * d * 2 + B * d * 4 + B * 3 * H * d * 2 * 2 +
                           B * s->nsplit * (H * d + 2 * H) * 4 * 2 + B * d * ws;
    if (which == WM_KERNEL_CROSS_ATTN) {
        // one layer: K and V rows of every utterance once + q in + partials out
        *bytes = m->xattn ? x_layer : B * 2.0 * c.n_audio_ctx * d * ks + B * d * 4 + B * s->nsplit * (d + 2 * H) * 4;
    } else if (which == WM_KERNEL_DECODE_STEP || which == WM_KERNEL_DECODE_STEP_SHARED) {
        // every weight once per step, KV once per utterance, KV write; logits are NOT materialised
        // (fused argmax: only B x ceil(V/128) (value, index) partials are written and re-read)
        const double f = c.ffn, L = c.n_layers, V = c.vocab;
        const double p_blk = 8 * d * d + 2 * f * d + (4 + 4 + 1 + 1 + 6) * d + f;  // 2 attn (4 mats each) + mlp + biases + 3 LN
        const double t = s->host_len > 0 ? s->host_len : BENCH_STEP_LEN;
        *bytes = ws * (L * (8 * d * d + 2 * f * d) + V * d) + 4 * (L * (p_blk - 8 * d * d - 2 * f * d) + 2 * d) +
                 B * L * 2 * d * ks * (c.n_audio_ctx + t) + B * L * 2 * d * ks + B * s->npart * 8.0 * 2 + B * 4;
        if (m->xattn)  // X and the bf16 Wk / Wv in place of the cross K/V cache (and the decoder-dtype Wk / Wv counted above)
            *bytes += L * (x_layer - B * 2.0 * c.n_audio_ctx * d * ks - 2 * d * d * ws);
    } else if (which == WM_KERNEL_ENCODER) {
        *bytes = 0;  // MFMA-bound: see wm_bench_flops in DESIGN.md
    } else {
        return fail(WM_E_ARG, "unknown kernel id %d", which);
    }
    return 0;
}

extern "C" int wm_bench_kernel(wm_model* m, wm_state* s, int which, int reps, float* avg_us) {
    if (!m || !s || !avg_us || reps <= 0) return fail(WM_E_ARG, "bad argument");
    WMCHK(check_state(m, s, -1));
    if (!s->has_cross) return fail(WM_E_STATE, "state has no cross K/V (call wm_encode first)");
    HIPCHK(hipSetDevice(m->device));
    hipStream_t st = m->stream;
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    const int L = m->cfg.dims.n_layers;
#ifdef WM_DEV
    // phase stamps in groups of 8 (100 MHz clock): per phase the sum / max of the us after the first group's entry; returns the groups seen
    auto phase_stats = [](const std::vector<long long>& h, int nphase, double* av, double* mx) {
        long long t0 = -1;
        for (size_t g = 0; g < h.size() / 8; ++g) if (h[g * 8] > 0 && (t0 < 0 || h[g * 8] < t0)) t0 = h[g * 8];
        int n = 0;
        for (size_t g = 0; g < h.size() / 8; ++g) {
            if (h[g * 8] <= 0) continue;
            ++n;
            for (int k = 0; k < nphase; ++k) {
                const double us = (double)(h[g * 8 + k] - t0) / 100.0;
                av[k] += us;
                mx[k] = std::max(mx[k], us);
            }
        }
        return n;
    };
#endif
    if (which == WM_KERNEL_CROSS_ATTN) {
        // m->xattn: absorb + X sweep + merge / V-apply, everything that replaces attn_decode + attn_combine (wm_bench_bytes prices
        // the same three launches).  Every layer reads the SAME X (73.7 MB at B = 64), so after the first launch the stream is
        // served from the 256 MB Infinity Cache — as it is inside a decode step, where the four layers re-read it.
        const DecView v = whole_batch(m, s);
        const int TD = dec_dtype(m->cfg);
        auto one = [&](int l) -> int {
            WMCHK(launch_cross_attn(m, s, l, v, 1));
            return m->xattn ? cross_attn_merge(m, s, l, v, 1, s->dattn.p, TD) : 0;
        };
        for (int i = 0; i < L; ++i) WMCHK(one(i));  // warm-up
        HIPCHK(hipEventRecord(e0, st));
        for (int i = 0; i < reps; ++i) WMCHK(one(i % L));  // fp32 K/V: cycles the layers, 4 x 295 MB > 256 MB L3
        HIPCHK(hipEventRecord(e1, st));
    } else if (which == WM_KERNEL_DECODE_STEP || which == WM_KERNEL_DECODE_STEP_SHARED) {
        s->shares_chip = which == WM_KERNEL_DECODE_STEP_SHARED;  // the K/V stream as pipelined passes launch it
        // on the state's own decode stream, as the transcribe loop runs it: several states can be timed concurrently
        // from several host threads (bench.py: four chains in flight)
        const int len0 = s->host_len > 0 ? s->host_len : BENCH_STEP_LEN;  // the cache length wm_bench_bytes prices
        HIPCHK(hipStreamSynchronize(m->stream));  // wm_encode ran there
        const bool own = s->lanes.size() == 1;      // (WM_DEC_LANES > 1: whole batch on the model stream as before)
        if (own) st = s->lanes[0].st;
        const DecView v{0, s->B, st, own ? s->lanes[0].ctl : s->ctl.as<StepCtl>()};
        launch_set_step(v.ctl, len0, 1, nullptr, 0, nullptr, 0, s->B, st);
        DecPass step;  // the bare step: embeds its input, logits partials with no mask
        step.logits = Logits::partials;
        WMCHK(decode_core(m, s, v, step));
        // timed as the transcribe loop runs it: a captured graph of the step, replayed (cache length held constant)
        hipGraph_t g = nullptr;
        hipGraphExec_t ge = nullptr;
        HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        const int crc = decode_core(m, s, v, step);
        const hipError_t cap = hipStreamEndCapture(st, &g);
        if (crc) {
            if (g) (void)hipGraphDestroy(g);
            return crc;
        }
        HIPCHK(cap);
        HIPCHK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
        (void)hipGraphDestroy(g);
        HIPCHK(hipGraphLaunch(ge, st));
        HIPCHK(hipEventRecord(e0, st));
        for (int i = 0; i < reps; ++i) HIPCHK(hipGraphLaunch(ge, st));
        HIPCHK(hipEventRecord(e1, st));
        HIPCHK(hipEventSynchronize(e1));
        (void)hipGraphExecDestroy(ge);
        s->shares_chip = false;
#ifdef WM_DEV
    } else if (which == 41 || which == 42) {  // developer: phase stamps of one LN1 + QKV (41) / O-proj (42) launch
        const wm_dims& c = m->cfg.dims;
        const int T = dec_dtype(m->cfg);
        DecLayer& w0 = m->dec[0];
        DevBuf dbg;
        WMCHK(dbg.alloc((size_t)4096 * 16 * 8 * 8, true));
        const DecView v = whole_batch(m, s);  // layer 0's launch as a single-position pass over the whole batch wires it
        DecLinearParams p = which == 41 ? qkv_block(m, s, v, 0, 1) : proj_residual_block(m, s, v, 1, s->dattn.as<float>(), c.d_model, w0.so_w, w0.so_b);
        launch_set_step(s->ctl.as<StepCtl>(), 10, 1, nullptr, 0, nullptr, 0, s->B, st);
        for (int i = 0; i < 3; ++i) { WMCHK(dec_linear_dispatch(T, p, st)); if (!wm_env("WM_STAMP_NO_STREAM")) WMCHK(launch_cross_attn(m, s, i, whole_batch(m, s), 1)); }
        p.dbg = dbg.as<long long>();
        HIPCHK(hipEventRecord(e0, st));
        WMCHK(dec_linear_dispatch(T, p, st));
        HIPCHK(hipEventRecord(e1, st));
        HIPCHK(hipEventSynchronize(e1));
        std::vector<long long> h((size_t)4096 * 16 * 8);
        HIPCHK(hipMemcpy(h.data(), dbg.p, h.size() * 8, hipMemcpyDeviceToHost));
        double mx[6] = {0}, av[6] = {0};
        const int n = phase_stats(h, 6, av, mx);
        fprintf(stderr, "[wm] dec_linear %s phases (us after the first wave's entry; mean / max over %d waves): entry %.2f/%.2f  loads issued %.2f/%.2f  operands ready %.2f/%.2f  MFMA + partial stored %.2f/%.2f  after barrier %.2f/%.2f  end %.2f/%.2f\n",
                which == 41 ? "LN1+QKV" : "O-proj", n, av[0] / n, mx[0], av[1] / n, mx[1], av[2] / n, mx[2], av[3] / n, mx[3], av[4] / n, mx[4], av[5] / n, mx[5]);
        dbg.release();
    } else if (which == 43) {  // developer: phase stamps of the encoder's QKV row-panel GEMM (layer 0) on the rows of the last encode
        const wm_dims& c = m->cfg.dims;
        const int T = m->cfg.compute_dtype;
        const int M = std::min(s->B, s->Bc) * c.n_audio_ctx;
        EncLayer& w0 = m->enc[0];
        GemmParams p{};
        p.A = s->xn.p; p.W = w0.qkv_w.p; p.C = s->qkv.p; p.M = M; p.N = 3 * c.d_model; p.K = c.d_model;
        p.lda = c.d_model; p.ldw = c.d_model; p.ldc = 3 * c.d_model; p.bias = w0.qkv_b.as<float>();
        if (!gemm_nt_fuses_layernorm(T == WM_F32 ? 4 : 2, p, 1)) return fail(WM_E_ARG, "this configuration does not run the row-panel kernel");
        for (int i = 0; i < 3; ++i) WMCHK(gemm_dispatch(T, T, p, 1, st));
        DevBuf dbg;
        WMCHK(dbg.alloc((size_t)512 * 96 * 8, true));
        p.dbg = dbg.as<long long>();
        HIPCHK(hipEventRecord(e0, st));
        WMCHK(gemm_dispatch(T, T, p, 1, st));
        HIPCHK(hipEventRecord(e1, st));
        HIPCHK(hipEventSynchronize(e1));
        std::vector<long long> h((size_t)512 * 96);
        HIPCHK(hipMemcpy(h.data(), dbg.p, h.size() * 8, hipMemcpyDeviceToHost));
        double wait = 0, issue = 0, comp = 0, epi = 0, gap = 0, unit = 0;
        int ns = 0, nu = 0, ng = 0;
        for (int g = 0; g < 512; ++g)
            for (int uu = 1; uu < 3; ++uu) {  // second and third unit of each workgroup (the first carries the panel load)
                const long long* d = &h[(size_t)g * 96 + uu * 32];
                if (d[0] <= 0 || d[25] <= 0) continue;
                for (int t = 0; t < 6; ++t) {
                    wait += (double)(d[t * 4 + 1] - d[t * 4 + 0]);
                    issue += (double)(d[t * 4 + 2] - d[t * 4 + 1]);
                    comp += (double)(d[t * 4 + 3] - d[t * 4 + 2]);
                    if (t > 0) { gap += (double)(d[t * 4] - d[t * 4 - 1]); ++ng; }
                    ++ns;
                }
                epi += (double)(d[25] - d[24]);
                unit += (double)(d[25] - d[0]);
                ++nu;
            }
        if (ns)
            fprintf(stderr, "[wm] row-panel QKV, wave 0, per 64-k stage (ns): wait + barrier %.0f  DMA issue %.0f  fragment reads + 32 MFMAs issued %.0f  to next top %.0f | "
                            "per unit: epilogue %.0f, whole unit %.0f (%d stages, %d units)\n",
                    wait / ns * 10, issue / ns * 10, comp / ns * 10, ng ? gap / ng * 10 : 0.0, epi / nu * 10, unit / nu * 10, ns, nu);
        dbg.release();
    } else if (which == 40) {  // developer: phase stamps of one logits launch (after a few warm ones), printed to stderr
        const int T = dec_dtype(m->cfg);
        DevBuf dbg;
        const int nwg = s->npart;
        WMCHK(dbg.alloc((size_t)nwg * 8 * 8 * 8, true));
        const VocabHead vh = vocab_head(m);
        DecLinearParams p = linear_block(s->dx.as<float>(), vh.ln_g, vh.ln_b, vh.emb, nullptr, vh.vocab, vh.d_model, s->B, nullptr, m->Vpad);
        p.amax_val = s->amax_val.as<float>(); p.amax_idx = s->amax_idx.as<int>(); p.amax_stride = s->npart;
        for (int i = 0; i < 3; ++i) { DISPATCH_DT(T, TT, (void)launch_dec_logits<TT>(p, st)); WMCHK(launch_cross_attn(m, s, i, whole_batch(m, s), 1)); }
        p.dbg = dbg.as<long long>();
        HIPCHK(hipEventRecord(e0, st));
        DISPATCH_DT(T, TT, (void)launch_dec_logits<TT>(p, st));
        HIPCHK(hipEventRecord(e1, st));
        HIPCHK(hipEventSynchronize(e1));
        std::vector<long long> h((size_t)nwg * 64);
        HIPCHK(hipMemcpy(h.data(), dbg.p, h.size() * 8, hipMemcpyDeviceToHost));
        double mx[8] = {0, 0, 0, 0, 0, 0, 0, 0}, av[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const int n = phase_stats(h, 7, av, mx);
        fprintf(stderr, "[wm] logits phases (us after the first wave's entry; mean / max over %d waves): entry %.2f/%.2f  loads issued + staged %.2f/%.2f  after barrier %.2f/%.2f  MFMA done %.2f/%.2f  end %.2f/%.2f\n",
                n, av[0] / n, mx[0], av[1] / n, mx[1], av[2] / n, mx[2], av[3] / n, mx[3], av[4] / n, mx[4]);
        fprintf(stderr, "[wm]   gamma/beta + activations arrived (own wave) %.2f/%.2f  all waves of the workgroup %.2f/%.2f\n", av[5] / n, mx[5], av[6] / n, mx[6]);
        dbg.release();
#endif
    } else if (which == WM_KERNEL_ENCODER) {
        if (!s->last_mel) return fail(WM_E_STATE, "no mel was encoded into this state");
        WMCHK(run_encoder(m, s, s->last_mel, s->B, st, nullptr, 0, false));  // as the transcribe paths run it
        HIPCHK(hipEventRecord(e0, st));
        for (int i = 0; i < reps; ++i) WMCHK(run_encoder(m, s, s->last_mel, s->B, st, nullptr, 0, false));
        HIPCHK(hipEventRecord(e1, st));
    } else {
        return fail(WM_E_ARG, "unknown kernel id %d", which);
    }
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *avg_us = ms * 1000.0f / (float)reps;
    return 0;
}
