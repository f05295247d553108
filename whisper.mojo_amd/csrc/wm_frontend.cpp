// wm_frontend.cpp — the log-mel front end for 30 s and for long audio, its wm_op_* hooks, the _pcm transcribe entries and the resampler.
#include "wm_runtime.h"

// ---- log-mel front end: 16 kHz PCM -> [n_mels, n_frames]  (export_weights.py:100-116 delegates this to
// HF WhisperProcessor = transformers feature_extraction_whisper._np_extract_fbank_features)
static double hz_to_mel_slaney(double f) { return f >= 1000.0 ? 15.0 + std::log(f / 1000.0) * (27.0 / std::log(6.4)) : 3.0 * f / 200.0; }
static double mel_to_hz_slaney(double m) { return m >= 15.0 ? 1000.0 * std::exp(std::log(6.4) / 27.0 * (m - 15.0)) : 200.0 * m / 3.0; }

// The front end's four tables for n_mels filters, built once on the host in float64 and rounded once: the periodic Hann window [400],
// the real-DFT basis [512][416] (cos at row k, -sin at row 256 + k, k < 201; every other entry 0), the slaney filter bank
// [201][n_mels] and, per filter, the interval [lo, hi) of bins outside which it is 0 (band [n_mels][2]; an empty filter gives 0, 0).
static const double FE_PI = 3.14159265358979323846;
static void frontend_window(std::vector<float>& window) {
    window.assign(FE_NFFT, 0.f);
    for (int n = 0; n < FE_NFFT; ++n) window[n] = (float)(0.5 - 0.5 * std::cos(2.0 * FE_PI * n / FE_NFFT));  // periodic Hann
}
static void frontend_tables(int n_mels, std::vector<float>& window, std::vector<float>& dft, std::vector<float>& fb, std::vector<int>& band) {
    const double PI = FE_PI;
    frontend_window(window);
    dft.assign((size_t)512 * 416, 0.f);
    fb.assign((size_t)FE_NFREQ * n_mels, 0.f);
    for (int k = 0; k < FE_NFREQ; ++k)
        for (int n = 0; n < FE_NFFT; ++n) {
            const double ang = 2.0 * PI * (double)((k * n) % FE_NFFT) / FE_NFFT;
            dft[(size_t)k * 416 + n] = (float)std::cos(ang);
            dft[(size_t)(256 + k) * 416 + n] = (float)(-std::sin(ang));
        }
    // slaney-scale, slaney-normalised triangular filters (transformers.audio_utils.mel_filter_bank)
    std::vector<double> ff(n_mels + 2);
    const double m0 = hz_to_mel_slaney(0.0), m1 = hz_to_mel_slaney(8000.0);
    for (int i = 0; i < n_mels + 2; ++i) ff[i] = mel_to_hz_slaney(m0 + (m1 - m0) * i / (n_mels + 1));
    band.assign(2 * (size_t)n_mels, 0);
    for (int mm = 0; mm < n_mels; ++mm) {
        int lo = FE_NFREQ, hi = 0;
        const double enorm = 2.0 / (ff[mm + 2] - ff[mm]);
        for (int k = 0; k < FE_NFREQ; ++k) {
            const double f = 8000.0 * k / (FE_NFREQ - 1);
            const double down = (f - ff[mm]) / (ff[mm + 1] - ff[mm]), up = (ff[mm + 2] - f) / (ff[mm + 2] - ff[mm + 1]);
            const double v = std::max(0.0, std::min(down, up)) * enorm;
            fb[(size_t)k * n_mels + mm] = (float)v;
            if (v > 0.0) {
                lo = std::min(lo, k);
                hi = std::max(hi, k + 1);
            }
        }
        band[2 * mm] = lo < hi ? lo : 0;
        band[2 * mm + 1] = lo < hi ? hi : 0;
    }
}

int frontend_init(wm_model* m) {
    if (m->fe.ready) return 0;
    const wm_dims& c = m->cfg.dims;
    const int n_mels = c.n_mels, n_frames = 2 * c.n_audio_ctx, N = FE_HOP * n_frames, maxB = m->cfg.max_batch;
    std::vector<float> window, dft, fb;
    std::vector<int> band;
    frontend_tables(n_mels, window, dft, fb, band);
    WMCHK(upload(m->fe.window, window.data(), window.size(), WM_F32));
    WMCHK(upload(m->fe.dft, dft.data(), dft.size(), WM_F32));
    WMCHK(upload(m->fe.fb, fb.data(), fb.size(), WM_F32));
    WMCHK(m->fe.band.alloc(band.size() * 4));
    HIPCHK(hipMemcpy(m->fe.band.p, band.data(), band.size() * 4, hipMemcpyHostToDevice));
    const size_t ch = std::min(maxB, m->fe.chunk);
    const size_t rows = (ch * n_frames + 255) / 256 * 256 + 256;
    WMCHK(m->fe.pcm.alloc((size_t)maxB * N * 4, true));
    WMCHK(m->fe.lens.alloc((size_t)maxB * 4, true));
    WMCHK(m->fe.frames.alloc(rows * 416 * 4, true));
    WMCHK(m->fe.spec.alloc(rows * 512 * 4, true));
    WMCHK(m->fe.logtmp.alloc((size_t)maxB * n_mels * n_frames * 4));
    WMCHK(m->fe.mel.alloc((size_t)maxB * n_mels * n_frames * 4));
    m->fe.ready = true;
    return 0;
}

// pcm: host [B][stride] fp32 at 16 kHz; n_samples[b] valid samples (<= stride).  Result stays in m->fe.mel (device).
int frontend_run(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride) {
    if (!pcm || !n_samples || B <= 0 || stride <= 0) return fail(WM_E_ARG, "bad argument");
    if (B > m->cfg.max_batch) return fail(WM_E_ARG, "batch %d exceeds max_batch %d", B, m->cfg.max_batch);
    HIPCHK(hipSetDevice(m->device));
    WMCHK(frontend_init(m));
    const wm_dims& c = m->cfg.dims;
    const int n_frames = 2 * c.n_audio_ctx, N = FE_HOP * n_frames;
    hipStream_t st = m->stream;
    // pad / trim to the 30 s window: ONE strided upload of the common prefix, then a kernel zeroes each utterance's tail
    for (int b = 0; b < B; ++b)
        if (n_samples[b] < 0 || n_samples[b] > stride) return fail(WM_E_ARG, "n_samples[%d]=%d out of range", b, n_samples[b]);
    const size_t w = std::min(stride, N);
    if (w < (size_t)N) HIPCHK(hipMemsetAsync(m->fe.pcm.p, 0, (size_t)B * N * 4, st));
    HIPCHK(hipMemcpy2DAsync(m->fe.pcm.p, (size_t)N * 4, pcm, (size_t)stride * 4, w * 4, B, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(m->fe.lens.p, n_samples, (size_t)B * 4, hipMemcpyHostToDevice, st));
    launch_zero_tails(m->fe.pcm.as<float>(), m->fe.lens.as<int>(), B, N, st);
    return frontend_compute(m, B, m->fe.mel.as<float>());
}
// m->fe.pcm [B][N] (padded / trimmed to the window, on the device) -> mel_out [B][n_mels][n_frames] (device), on the model's stream
int frontend_compute(wm_model* m, int B, float* mel_out) {
    const wm_dims& c = m->cfg.dims;
    const int n_frames = 2 * c.n_audio_ctx, N = FE_HOP * n_frames;
    hipStream_t st = m->stream;
    for (int c0 = 0; c0 < B; c0 += m->fe.chunk) {
        const int bc = std::min(m->fe.chunk, B - c0);
        launch_frames(m->fe.pcm.as<float>() + (size_t)c0 * N, m->fe.frames.as<float>(), m->fe.window.as<float>(), bc, N, n_frames, FE_HOP, st);
        GemmParams p{};
        p.A = m->fe.frames.p;
        p.W = m->fe.dft.p;
        p.C = m->fe.spec.p;
        p.M = bc * n_frames;
        p.N = 512;
        p.K = 416;
        p.lda = 416;
        p.ldw = 416;
        p.ldc = 512;
        LCHK((launch_gemm_nt<float, float>(p, 1, st)));
        launch_mel_log(m->fe.spec.as<float>(), m->fe.fb.as<float>(), m->fe.band.as<int>(), m->fe.logtmp.as<float>() + (size_t)c0 * c.n_mels * n_frames,
                       bc, n_frames, c.n_mels, st);
    }
    launch_mel_norm(m->fe.logtmp.as<float>(), mel_out, B, c.n_mels * n_frames, st);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int wm_log_mel(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, float* mel_out) {
    if (!m) return fail(WM_E_ARG, "null model");
    WMCHK(frontend_run(m, pcm, n_samples, B, stride));
    const wm_dims& c = m->cfg.dims;
    if (mel_out) HIPCHK(hipMemcpyAsync(mel_out, m->fe.mel.p, (size_t)B * c.n_mels * 2 * c.n_audio_ctx * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return 0;
}

// ---- the front end's stages one at a time (known-answer tests; include/whisper_mi.h) -- each through the launcher the runtime uses
static const int FE_MAX_MELS = 128, FE_MAX_GRID_Y = 65535;
extern "C" int wm_op_fe_tables(int n_mels, float* window, float* dft, float* fb, int32_t* band) {
    if (!window || !dft || !fb || !band || n_mels < 1 || n_mels > FE_MAX_MELS) return fail(WM_E_ARG, "bad argument (1 <= n_mels <= %d)", FE_MAX_MELS);
    std::vector<float> w, d, f;
    std::vector<int> bd;
    frontend_tables(n_mels, w, d, f, bd);
    memcpy(window, w.data(), w.size() * 4);
    memcpy(dft, d.data(), d.size() * 4);
    memcpy(fb, f.data(), f.size() * 4);
    memcpy(band, bd.data(), bd.size() * 4);
    return 0;
}
extern "C" int wm_op_fe_frames(float* out, const float* pcm, const int32_t* n_samples, int B, int N, int n, int t0) {
    if (!out || !pcm || B <= 0 || B > FE_MAX_GRID_Y || N <= 200 || n <= 0 || t0 < 0)
        return fail(WM_E_ARG, "bad argument (B >= 1, N > 200, n >= 1, t0 >= 0)");
    if ((int64_t)t0 + n > N / FE_HOP)
        return fail(WM_E_ARG, "frames [%d, %lld) leave the %d frames of %d samples", t0, (long long)t0 + n, N / FE_HOP, N);
    if (n_samples)
        for (int b = 0; b < B; ++b)
            if (n_samples[b] < 0 || n_samples[b] > N) return fail(WM_E_ARG, "n_samples[%d]=%d out of range", b, n_samples[b]);
    std::vector<float> window;
    frontend_window(window);
    TmpDev tmp;
    DevBuf &dp = tmp.add(), &dl = tmp.add(), &dw = tmp.add(), &dout = tmp.add();
    const size_t n_out = ((size_t)B * n + 1) * 416;  // one guard row behind the last frame
    WMCHK(upload(dp, pcm, (size_t)B * N, WM_F32));
    WMCHK(upload(dw, window.data(), window.size(), WM_F32));
    WMCHK(upload(dout, out, n_out, WM_F32));  // in and out: what the kernel does not store keeps the caller's value
    if (n_samples) {
        WMCHK(upload_bytes(dl, n_samples, (size_t)B * 4));
        launch_zero_tails(dp.as<float>(), dl.as<int>(), B, N, nullptr);
    }
    launch_frames(dp.as<float>(), dout.as<float>(), dw.as<float>(), B, N, n, FE_HOP, nullptr, t0);
    HIPCHK(hipGetLastError());
    return download_f32(out, dout, n_out, WM_F32);
}
extern "C" int wm_op_fe_mel_log(float* logmel, const float* spec, int B, int n, int n_mels, int out_frames, int t_out) {
    if (!logmel || !spec || B <= 0 || B > FE_MAX_GRID_Y || n <= 0 || n_mels < 1 || n_mels > FE_MAX_MELS || t_out < 0)
        return fail(WM_E_ARG, "bad argument (B >= 1, n >= 1, 1 <= n_mels <= %d, t_out >= 0)", FE_MAX_MELS);
    if (out_frames <= 0 || (int64_t)t_out + n > out_frames)
        return fail(WM_E_ARG, "frames [%d, %lld) leave the row of %d", t_out, (long long)t_out + n, out_frames);
    std::vector<float> window, dft, fb;
    std::vector<int> band;
    frontend_tables(n_mels, window, dft, fb, band);
    TmpDev tmp;
    DevBuf &ds = tmp.add(), &df = tmp.add(), &db = tmp.add(), &dout = tmp.add();
    const size_t n_out = (size_t)B * n_mels * out_frames;
    WMCHK(upload(ds, spec, (size_t)B * n * 512, WM_F32));
    WMCHK(upload(df, fb.data(), fb.size(), WM_F32));
    WMCHK(upload_bytes(db, band.data(), band.size() * 4));
    WMCHK(upload(dout, logmel, n_out, WM_F32));  // in and out
    launch_mel_log(ds.as<float>(), df.as<float>(), db.as<int>(), dout.as<float>(), B, n, n_mels, nullptr, out_frames, t_out);
    HIPCHK(hipGetLastError());
    return download_f32(logmel, dout, n_out, WM_F32);
}
extern "C" int wm_op_fe_mel_norm(float* out, const float* logmel, int B, int64_t n, int long_mode) {
    if (!out || !logmel || B <= 0 || B > FE_MAX_GRID_Y || n <= 0 || (long_mode != 0 && long_mode != 1)) return fail(WM_E_ARG, "bad argument");
    if (n > INT32_MAX) return fail(WM_E_ARG, "n = %lld exceeds 2^31 - 1", (long long)n);
    TmpDev tmp;
    DevBuf &dx = tmp.add(), &dy = tmp.add(), &dpart = tmp.add();
    WMCHK(upload(dx, logmel, (size_t)B * n, WM_F32));
    if (long_mode) {
        WMCHK(dpart.alloc((size_t)B * 256 * 4));
        launch_mel_norm_long(dx.as<float>(), dpart.as<float>(), B, (size_t)n, nullptr);  // in place
    } else {
        WMCHK(dy.alloc((size_t)B * n * 4));
        launch_mel_norm(dx.as<float>(), dy.as<float>(), B, (int)n, nullptr);
    }
    HIPCHK(hipGetLastError());
    return download_f32(out, long_mode ? dx : dy, (size_t)B * n, WM_F32);
}
extern "C" int wm_op_window_gather(float* out, const float* mel, const int32_t* items, int rows, int B, int n_mels, int F, int W) {
    if (!out || !mel || !items || rows <= 0 || rows > FE_MAX_GRID_Y || B <= 0 || n_mels < 1 || n_mels > FE_MAX_MELS || F <= 0 || W <= 0)
        return fail(WM_E_ARG, "bad argument");
    for (int r = 0; r < rows; ++r) {
        const int32_t* t = items + 3 * (size_t)r;
        if (t[0] < 0 || t[0] >= B || t[1] < 0 || t[2] < 0 || t[2] > W || (int64_t)t[1] + t[2] > F)
            return fail(WM_E_ARG, "item %d = (%d, %d, %d) leaves mel [%d][%d][%d] or the window of %d frames", r, t[0], t[1], t[2], B, n_mels, F, W);
    }
    TmpDev tmp;
    DevBuf &dm = tmp.add(), &di = tmp.add(), &dout = tmp.add();
    const size_t n_out = (size_t)rows * n_mels * W;
    WMCHK(upload(dm, mel, (size_t)B * n_mels * F, WM_F32));
    WMCHK(upload_bytes(di, items, (size_t)rows * 3 * 4));
    WMCHK(upload(dout, out, n_out, WM_F32));  // in and out
    launch_window_gather(dm.as<float>(), di.as<int>(), dout.as<float>(), rows, n_mels, F, W, nullptr);
    HIPCHK(hipGetLastError());
    return download_f32(out, dout, n_out, WM_F32);
}

extern "C" int wm_transcribe_pcm(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, const wm_decode_opts* o,
                                 int32_t* tokens_out, int32_t* n_tokens) {
    if (!m || !tokens_out || !n_tokens) return fail(WM_E_ARG, "bad argument");
    WMCHK(check_opts(m, o, B));
    WMCHK(frontend_run(m, pcm, n_samples, B, stride));  // same stream as the encoder: ordered, no host sync
    return run_now(m, PassAsk{m->fe.mel.as<float>(), 1, B, o}, PassOut{tokens_out, n_tokens});
}

// n_frames[b] = min(2·n_audio_ctx, ceil(n_samples[b] / 160)): the attention mask of WhisperFeatureExtractor
extern "C" int wm_transcribe_pcm_tt(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, const wm_decode_opts* o,
                                    int32_t* tokens_out, int32_t* n_tokens, float* token_times) {
    if (!m || !tokens_out || !n_tokens || !token_times || !n_samples || B <= 0) return fail(WM_E_ARG, "bad argument");
    WMCHK(check_opts(m, o, B));
    std::vector<int32_t> nf(B);
    for (int b = 0; b < B; ++b) nf[b] = (int32_t)std::min<long>(2L * m->cfg.dims.n_audio_ctx, ((long)n_samples[b] + FE_HOP - 1) / FE_HOP);
    std::vector<int32_t> cols;
    WMCHK(align_cols(m, nf.data(), B, cols));
    WMCHK(frontend_run(m, pcm, n_samples, B, stride));
    PassAsk ask{m->fe.mel.as<float>(), 1, B, o};
    ask.cols = &cols;
    return run_now(m, ask, PassOut{tokens_out, n_tokens, token_times});
}

// ---- any sample rate and int16 in: resampling to 16 kHz on the GPU --------------------------------------------------
// torchaudio.functional.resample(x, sr_in, 16000) with its defaults (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99): the
// taps are computed in float64 and rounded once; sr_in = 16000 is the identity (one tap of 1, as torchaudio returns its input).
static const int RS_RATE = 16000, RS_MAX_RATIO = 1024;
static int resample_ratio(int sr_in, int* orig, int* nw, int* width) {
    if (sr_in <= 0) return fail(WM_E_ARG, "sr_in = %d must be positive", sr_in);
    int a = sr_in, b = RS_RATE;
    while (b) {
        const int t = a % b;
        a = b, b = t;
    }
    const int64_t o = sr_in / a, n = RS_RATE / a;
    if (o > RS_MAX_RATIO || n > RS_MAX_RATIO)
        return fail(WM_E_ARG, "sr_in = %d: the reduced ratio %lld / %lld has a term above %d", sr_in, (long long)o, (long long)n, RS_MAX_RATIO);
    *orig = (int)o, *nw = (int)n;
    const double base = (double)std::min(o, n) * 0.99;
    *width = sr_in == RS_RATE ? 0 : (int)std::ceil(6.0 * (double)o / base);
    return 0;
}
// h [nw][2 * width + orig]
static void resample_taps_host(int orig, int nw, int width, std::vector<float>& h) {
    const int K = 2 * width + orig;
    h.assign((size_t)nw * K, 0.f);
    if (width == 0) {
        h[0] = 1.f;
        return;
    }
    const double PI = 3.14159265358979323846, base = (double)std::min(orig, nw) * 0.99, scale = base / (double)orig;
    for (int p = 0; p < nw; ++p)
        for (int k = 0; k < K; ++k) {
            double t = (-(double)p / (double)nw + (double)(k - width) / (double)orig) * base;
            t = std::min(6.0, std::max(-6.0, t));
            const double pt = PI * t, s = t == 0.0 ? 1.0 : std::sin(pt) / pt, c = std::cos(pt / 12.0);
            h[(size_t)p * K + k] = (float)(s * (c * c) * scale);
        }
}
static int resample_len(int64_t n_in, int orig, int nw, int64_t* n_out) {
    if (n_in < 0) return fail(WM_E_ARG, "n_in = %lld is negative", (long long)n_in);
    if (n_in > INT64_MAX / RS_MAX_RATIO - RS_MAX_RATIO) return fail(WM_E_SIZE, "n_in = %lld: the output length leaves 64 bits", (long long)n_in);
    *n_out = (n_in * nw + orig - 1) / orig;
    return 0;
}
extern "C" int wm_resample_len(int64_t n_in, int sr_in, int64_t* n_out) {
    if (!n_out) return fail(WM_E_ARG, "bad argument");
    int orig, nw, width;
    WMCHK(resample_ratio(sr_in, &orig, &nw, &width));
    return resample_len(n_in, orig, nw, n_out);
}
extern "C" int wm_op_resample_taps(int sr_in, float* taps, int64_t cap, int* orig, int* nw, int* width) {
    if (!orig || !nw || !width || cap < 0 || (cap > 0 && !taps)) return fail(WM_E_ARG, "bad argument");
    WMCHK(resample_ratio(sr_in, orig, nw, width));
    if (!taps) return 0;
    const int64_t need = (int64_t)*nw * (2 * *width + *orig);
    if (cap < need) return fail(WM_E_SIZE, "cap = %lld is smaller than the table of %lld taps", (long long)cap, (long long)need);
    std::vector<float> h;
    resample_taps_host(*orig, *nw, *width, h);
    memcpy(taps, h.data(), h.size() * 4);
    return 0;
}
// the table of one sr_in on the device, in the layout resample_kernel reads (wm_kernels.h ResampleParams)
static int resampler_build(wm_model::Frontend::Resampler& r, int sr_in) {
    WMCHK(resample_ratio(sr_in, &r.orig, &r.nw, &r.width));
    std::vector<float> h;
    resample_taps_host(r.orig, r.nw, r.width, h);
    const int K = 2 * r.width + r.orig;
    std::vector<int32_t> span(2 * (size_t)r.nw, 0);
    int most = 1;
    for (int p = 0; p < r.nw; ++p) {
        int lo = K, hi = 0;
        for (int k = 0; k < K; ++k)
            if (h[(size_t)p * K + k] != 0.f) lo = std::min(lo, k), hi = k + 1;
        if (lo < hi) span[2 * p] = lo, span[2 * p + 1] = hi - lo;
        most = std::max(most, span[2 * p + 1]);
    }
    std::vector<float> compact((size_t)most * r.nw, 0.f);
    for (int p = 0; p < r.nw; ++p)
        for (int q = 0; q < span[2 * p + 1]; ++q) compact[(size_t)q * r.nw + p] = h[(size_t)p * K + span[2 * p] + q];
    WMCHK(r.taps.alloc(compact.size() * 4));
    WMCHK(r.span.alloc(span.size() * 4));
    HIPCHK(hipMemcpy(r.taps.p, compact.data(), compact.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(r.span.p, span.data(), span.size() * 4, hipMemcpyHostToDevice));
    r.frames = resample_frames(r.orig, r.nw, r.width);
    r.sr = sr_in;
    return 0;
}
// what both entries refuse before anything is launched; n_out [B] and the longest row's output length
static int resample_check(const void* in, int in_dtype, const int32_t* n_in, int B, int64_t stride_in, int sr_in, const void* out, int64_t stride_out,
                          int32_t* n_out, int64_t* longest) {
    if (!in || !out || !n_in || !n_out || B <= 0 || stride_in <= 0 || stride_out <= 0) return fail(WM_E_ARG, "bad argument");
    int orig, nw, width;
    WMCHK(resample_ratio(sr_in, &orig, &nw, &width));
    if (in_dtype != WM_F32 && in_dtype != WM_I16) return fail(WM_E_ARG, "in_dtype = %d is neither WM_F32 nor WM_I16", in_dtype);
    if (B > 65535) return fail(WM_E_ARG, "B = %d rows exceed 65535", B);
    *longest = 0;
    for (int b = 0; b < B; ++b) {
        if (n_in[b] < 0 || n_in[b] > stride_in) return fail(WM_E_ARG, "n_in[%d] = %d outside [0, stride_in = %lld]", b, n_in[b], (long long)stride_in);
        int64_t n = 0;
        WMCHK(resample_len(n_in[b], orig, nw, &n));
        if (n > INT32_MAX) return fail(WM_E_SIZE, "row %d resamples to %lld samples, more than 2^31 - 1", b, (long long)n);
        *longest = std::max(*longest, n);
    }
    if (*longest > stride_out) return fail(WM_E_SIZE, "stride_out = %lld is smaller than the longest row's %lld samples", (long long)stride_out, (long long)*longest);
    for (int b = 0; b < B; ++b) n_out[b] = (int32_t)(((int64_t)n_in[b] * nw + orig - 1) / orig);
    return 0;
}
static int resample_launch(const wm_model::Frontend::Resampler& r, const void* d_in, int in_dtype, const int* d_nin, int B, int64_t stride_in, float* d_out,
                           int64_t stride_out, int* d_nout, int64_t longest, hipStream_t st) {
    ResampleParams p{};
    p.x = d_in, p.y = d_out, p.n_in = d_nin, p.n_out = d_nout;
    p.stride_in = (size_t)stride_in, p.stride_out = (size_t)stride_out;
    p.taps = r.taps.as<float>(), p.span = r.span.as<int>();
    p.orig = r.orig, p.nw = r.nw, p.width = r.width, p.frames = r.frames;
    LCHK(launch_resample(p, in_dtype == WM_I16, B, longest, st));
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int wm_op_resample(float* out, const void* in, int in_dtype, const int32_t* n_in, int B, int64_t stride_in, int sr_in, int64_t stride_out,
                              int32_t* n_out) {
    if (!n_out) return fail(WM_E_ARG, "bad argument");
    int64_t longest = 0;
    std::vector<int32_t> no(std::max(B, 1));
    WMCHK(resample_check(in, in_dtype, n_in, B, stride_in, sr_in, out, stride_out, no.data(), &longest));
    wm_model::Frontend::Resampler r;
    TmpDev tmp;
    DevBuf &din = tmp.add(), &dout = tmp.add(), &dni = tmp.add(), &dno = tmp.add();
    const size_t es = in_dtype == WM_I16 ? 2 : 4, nin = (size_t)B * stride_in, nout = (size_t)B * stride_out;
    int rc = resampler_build(r, sr_in);
    auto run = [&]() -> int {
        WMCHK(upload_bytes(din, in, nin * es));
        WMCHK(upload_bytes(dout, out, nout * 4));  // in and out: a cell the kernel does not store keeps the caller's value
        WMCHK(upload_bytes(dni, n_in, (size_t)B * 4));
        WMCHK(upload_bytes(dno, n_out, (size_t)B * 4));
        WMCHK(resample_launch(r, din.p, in_dtype, dni.as<int>(), B, stride_in, dout.as<float>(), stride_out, dno.as<int>(), longest, nullptr));
        HIPCHK(hipMemcpy(out, dout.p, nout * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(n_out, dno.p, (size_t)B * 4, hipMemcpyDeviceToHost));  // what the kernel computed, not the host's copy
        return 0;
    };
    if (!rc) rc = run();
    r.taps.release();
    r.span.release();
    return rc;
}
static int resampler_get(wm_model* m, int sr_in, wm_model::Frontend::Resampler** out) {
    for (auto* r : m->fe.rs)
        if (r->sr == sr_in) {
            *out = r;
            return 0;
        }
    auto* r = new wm_model::Frontend::Resampler();
    const int rc = resampler_build(*r, sr_in);
    if (rc) {
        r->taps.release();
        r->span.release();
        delete r;
        return rc;
    }
    m->fe.rs.push_back(r);
    *out = r;
    return 0;
}
extern "C" int wm_resample_pcm(wm_model* m, const void* in, int in_dtype, int in_on_device, const int32_t* n_in, int B, int64_t stride_in, int sr_in,
                               float* out, int out_on_device, int64_t stride_out, int32_t* n_out) {
    if (!m) return fail(WM_E_ARG, "null model");
    if (!n_out) return fail(WM_E_ARG, "bad argument");
    int64_t longest = 0;
    std::vector<int32_t> no(std::max(B, 1));
    WMCHK(resample_check(in, in_dtype, n_in, B, stride_in, sr_in, out, stride_out, no.data(), &longest));
    if (stride_out > INT32_MAX) return fail(WM_E_SIZE, "stride_out = %lld exceeds 2^31 - 1", (long long)stride_out);
    HIPCHK(hipSetDevice(m->device));
    wm_model::Frontend::Resampler* r = nullptr;
    WMCHK(resampler_get(m, sr_in, &r));
    hipStream_t st = m->stream;
    TmpDev tmp;
    DevBuf &din = tmp.add(), &dout = tmp.add(), &dni = tmp.add(), &dno = tmp.add();
    const size_t es = in_dtype == WM_I16 ? 2 : 4, nin = (size_t)B * stride_in, nout = (size_t)B * stride_out;
    auto run = [&]() -> int {
        const void* d_in = in;
        float* d_out = out;
        if (!in_on_device) {
            WMCHK(din.alloc(nin * es));
            HIPCHK(hipMemcpyAsync(din.p, in, nin * es, hipMemcpyHostToDevice, st));
            d_in = din.p;
        }
        if (!out_on_device) {
            WMCHK(dout.alloc(nout * 4));
            d_out = dout.as<float>();
        }
        WMCHK(dni.alloc((size_t)B * 4));
        WMCHK(dno.alloc((size_t)B * 4));
        HIPCHK(hipMemcpyAsync(dni.p, n_in, (size_t)B * 4, hipMemcpyHostToDevice, st));
        WMCHK(resample_launch(*r, d_in, in_dtype, dni.as<int>(), B, stride_in, d_out, stride_out, dno.as<int>(), longest, st));
        launch_zero_tails(d_out, dno.as<int>(), B, (int)stride_out, st);  // the model path hands on rows that are zero past their length
        HIPCHK(hipGetLastError());
        if (!out_on_device) HIPCHK(hipMemcpyAsync(out, dout.p, nout * 4, hipMemcpyDeviceToHost, st));
        return 0;
    };
    const int rc = run();
    const std::string err = g_err;
    const hipError_t e = hipStreamSynchronize(st);  // the scratch is released on return, and no[] is the caller's from here
    if (rc) {
        g_err = err;
        return rc;
    }
    if (e != hipSuccess) return fail(WM_E_HIP, "hipStreamSynchronize: %s", hipGetErrorString(e));
    std::copy(no.begin(), no.begin() + B, n_out);
    return 0;
}

// Log-mel of long audio into m->lf.mel [B][n_mels][stride / 160] (device): the 30 s path's kernels over chunks of frames of all
// utterances at once, so frames / spec stay one chunk however long the audio; then the two-stage max and the clamp / rescale.
static const int LONG_FE_ROWS = 16 * 3000;  // frames per DFT GEMM (the 30 s path's largest chunk)
int frontend_long_run(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, int32_t* n_frames_out) {
    if (!pcm || !n_samples || B <= 0 || stride <= 200) return fail(WM_E_ARG, "bad argument (B >= 1, stride > 200 samples)");
    for (int b = 0; b < B; ++b)
        if (n_samples[b] < 0 || n_samples[b] > stride) return fail(WM_E_ARG, "n_samples[%d]=%d out of range", b, n_samples[b]);
    HIPCHK(hipSetDevice(m->device));
    WMCHK(frontend_init(m));
    const int n_mels = m->cfg.dims.n_mels, F = stride / FE_HOP;
    hipStream_t st = m->stream;
    wm_model::LongForm& L = m->lf;
    const int nt = std::max(32, std::min((F + 31) / 32 * 32, LONG_FE_ROWS / B / 32 * 32));  // frames per chunk and utterance
    const size_t rows = ((size_t)B * nt + 255) / 256 * 256 + 256;
    if (!L.frames.p || L.frames.bytes < rows * 416 * 4) WMCHK(L.frames.alloc(rows * 416 * 4, true));
    if (!L.spec.p || L.spec.bytes < rows * 512 * 4) WMCHK(L.spec.alloc(rows * 512 * 4, true));
    WMCHK(grow(L.pcm, (size_t)B * stride * 4));
    WMCHK(grow(L.lens, (size_t)B * 4));
    WMCHK(grow(L.part, (size_t)B * 256 * 4));
    WMCHK(grow(L.mel, (size_t)B * n_mels * F * 4));
    HIPCHK(hipMemcpyAsync(L.pcm.p, pcm, (size_t)B * stride * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(L.lens.p, n_samples, (size_t)B * 4, hipMemcpyHostToDevice, st));
    launch_zero_tails(L.pcm.as<float>(), L.lens.as<int>(), B, stride, st);  // HF pads with zeros to the longest recording
    for (int t0 = 0; t0 < F; t0 += nt) {
        const int n = std::min(nt, F - t0);
        launch_frames(L.pcm.as<float>(), L.frames.as<float>(), m->fe.window.as<float>(), B, stride, n, FE_HOP, st, t0);
        GemmParams p{};
        p.A = L.frames.p;
        p.W = m->fe.dft.p;
        p.C = L.spec.p;
        p.M = B * n;
        p.N = 512;
        p.K = 416;
        p.lda = 416;
        p.ldw = 416;
        p.ldc = 512;
        LCHK((launch_gemm_nt<float, float>(p, 1, st)));
        launch_mel_log(L.spec.as<float>(), m->fe.fb.as<float>(), m->fe.band.as<int>(), L.mel.as<float>(), B, n, n_mels, st, F, t0);
    }
    launch_mel_norm_long(L.mel.as<float>(), L.part.as<float>(), B, (size_t)n_mels * F, st);
    HIPCHK(hipGetLastError());
    if (n_frames_out)
        for (int b = 0; b < B; ++b) n_frames_out[b] = std::min((n_samples[b] + FE_HOP - 1) / FE_HOP, F);
    return 0;
}

extern "C" int wm_log_mel_long(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, float* mel_out, int32_t* n_frames_out) {
    if (!m) return fail(WM_E_ARG, "null model");
    const int rc = frontend_long_run(m, pcm, n_samples, B, stride, n_frames_out);
    if (rc) {
        (void)hipStreamSynchronize(m->stream);
        long_release(m);
        return rc;
    }
    hipError_t e = hipSuccess;
    if (mel_out)
        e = hipMemcpyAsync(mel_out, m->lf.mel.p, (size_t)B * m->cfg.dims.n_mels * (stride / FE_HOP) * 4, hipMemcpyDeviceToHost, m->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
    long_release(m);
    if (e != hipSuccess) return fail(WM_E_HIP, "wm_log_mel_long: %s", hipGetErrorString(e));
    return 0;
}
