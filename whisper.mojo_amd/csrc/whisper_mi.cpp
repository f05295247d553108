// whisper_mi.cpp — host runtime behind the C-ABI of include/whisper_mi.h (compiled with hipcc).
//
// One wm_model per GPU: weights resident in HBM in kernel-friendly layouts, one HIP stream, no per-op allocation
// (the reference zero-fills a fresh heap Tensor for every intermediate, whisper_tensor.mojo:17-23; here every
// buffer belongs to a preallocated per-state arena).  The greedy loop of Whisper.transcribe (whisper.mojo:184-223)
// runs with the token feedback entirely on the device.
#include "../../include/whisper_mi.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <set>
#include <thread>
#include <string>
#include <unordered_set>
#include <vector>

#include "wm_runtime.h"

using namespace wm;

// ------------------------------------------------------------------------------------------------------------
thread_local std::string g_err;
int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

extern "C" const char* wm_last_error(void) { return g_err.c_str(); }
extern "C" int wm_abi_version(void) { return WM_ABI_VERSION; }

int launch_rc(int st) {
    if (st == wm::WM_LAUNCH_OK) return 0;
    return fail(st == wm::WM_LAUNCH_HIP ? WM_E_HIP : WM_E_ARG, "%s", wm::launch_last_refusal());
}

// Developer timeline (WM_TRACE_EVENTS=1): HIP events recorded on the library's streams at pass / phase boundaries and
// printed, sorted on the GPU clock, when the model is freed.  The profiler serialises concurrent queues; events do not.
struct TraceMark {
    hipEvent_t ev;
    std::string label;
};
static std::vector<TraceMark> g_trace;
static bool trace_events_on() {
    static const bool on = wm_env("WM_TRACE_EVENTS") != nullptr;
    return on;
}
void trace_mark(hipStream_t st, const char* fmt, ...) {
    if (!trace_events_on() || g_trace.size() > 200000) return;
    char buf[128];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return;
    (void)hipEventRecord(e, st);
    g_trace.push_back({e, buf});
}
static void trace_dump() {
    if (g_trace.empty()) return;
    (void)hipDeviceSynchronize();
    std::vector<std::pair<float, std::string>> rows;
    for (auto& t : g_trace) {
        float ms = 0.f;
        const hipError_t e = hipEventElapsedTime(&ms, g_trace[0].ev, t.ev);
        if (e == hipSuccess)
            rows.push_back({ms, t.label});
        else
            fprintf(stderr, "[wm-trace] %s: %s\n", t.label.c_str(), hipGetErrorString(e));
    }
    for (auto& t : g_trace) (void)hipEventDestroy(t.ev);
    g_trace.clear();
    std::sort(rows.begin(), rows.end());
    for (auto& r : rows) fprintf(stderr, "[wm-trace] %10.3f ms  %s\n", r.first, r.second.c_str());
}

int upload(DevBuf& b, const float* h, size_t n, int dt) {
    WMCHK(b.alloc(n * dt_size(dt)));
    if (dt == WM_F32) {
        HIPCHK(hipMemcpy(b.p, h, n * 4, hipMemcpyHostToDevice));
    } else {
        std::vector<uint16_t> tmp(n);
        if (dt == WM_BF16)
            for (size_t i = 0; i < n; ++i) tmp[i] = f32_to_bf16_host(h[i]);
        else
            for (size_t i = 0; i < n; ++i) tmp[i] = f32_to_f16_host(h[i]);
        HIPCHK(hipMemcpy(b.p, tmp.data(), n * 2, hipMemcpyHostToDevice));
    }
    return 0;
}

// Every live wm_state: a handle that is not in here (already freed — e.g. by wm_model_free, which owns the states created
// on it — or never valid) is rejected instead of dereferenced.
static std::mutex g_states_mu;
static std::unordered_set<const void*> g_live_states;
bool state_is_live(const void* s) {
    std::lock_guard<std::mutex> lk(g_states_mu);
    return s && g_live_states.count(s) != 0;
}

// ------------------------------------------------------------------------------------------------------------
// C = LN(x) W^T (+ epilogue of p): p.A names the scratch for the normalised rows.  The A-stationary GEMM normalises the fp32 rows
// while it loads them (no LayerNorm launch, no 16-bit copy through HBM); every other shape runs layernorm_rows first.
int ln_then_gemm(int dt_in, int dt_out, GemmParams p, const float* x, const float* g, const float* b, hipStream_t st) {
    if (gemm_nt_fuses_layernorm(dt_in == WM_F32 ? 4 : 2, p, 1)) {
        p.A = x;
        p.ln_g = g;
        p.ln_b = b;
    } else {
        DISPATCH_DT(dt_in, TT, launch_layernorm_rows<TT>(x, g, b, const_cast<void*>(p.A), nullptr, p.M, p.K, 1e-5f, st));
    }
    return gemm_dispatch(dt_in, dt_out, p, 1, st);
}
// 0 or a WM_E_* status with wm_last_error set (a shape the kernels refuse: nothing was launched)
int gemm_dispatch(int dt_in, int dt_out, const GemmParams& p, int batch, hipStream_t st) {
    int rc;
    if (dt_in == WM_F32) {
        rc = launch_gemm_nt<float, float>(p, batch, st);
    } else if (dt_in == WM_BF16) {
        rc = dt_out == WM_F32 ? launch_gemm_nt<bf16, float>(p, batch, st) : launch_gemm_nt<bf16, bf16>(p, batch, st);
    } else {
        rc = dt_out == WM_F32 ? launch_gemm_nt<f16, float>(p, batch, st) : launch_gemm_nt<f16, f16>(p, batch, st);
    }
    return launch_rc(rc);
}

extern "C" size_t wm_weight_count(const wm_dims* c) { return wm_synth_count(c); }
extern "C" size_t wm_synth_weights(const wm_dims* dims, uint64_t seed, float* out) { return wm_synth_fill(dims, seed, out); }
extern "C" void wm_synth_mel_host(uint64_t seed, int n_mels, int n_frames, float* out) {
    wm_synth_mel(seed, n_mels, n_frames, out);
}

static int check_cfg(const wm_config* c) {
    const wm_dims& d = c->dims;
    if (d.d_model <= 0 || d.n_heads <= 0 || d.d_model != d.n_heads * 64)
        return fail(WM_E_ARG, "d_model must equal n_heads*64 (got %d, %d)", d.d_model, d.n_heads);
    // Whisper-small (d_model 768, 12 heads, ffn 3072) and Whisper-medium (d_model 1024, 16 heads, ffn 4096) are the two shapes past 8
    // heads: their cross-attention runs on the K/V cache (m->xattn stays <= 8 heads), their fc2 on the K-long form of the skinny linear
    // (launch_dec_linear_long)
    const bool small = d.d_model == 768 && d.n_heads == 12, medium = d.d_model == 1024 && d.n_heads == 16;
    if (d.n_heads > 8 && !small && !medium)
        return fail(WM_E_ARG, "n_heads > 8 not supported (except 12 heads at d_model 768 and 16 heads at d_model 1024)");
    if (d.d_model % 128 || d.ffn % 128) return fail(WM_E_ARG, "d_model and ffn must be multiples of 128");
    // what the decode kernels are instantiated for: the logits kernel keeps d_model/128 in {1, 3, 4, 6, 8} k-panels
    // (kernels_decoder.hip launch_dec_logits), the skinny linears split K/32 k-steps over <= 16 waves x <= 4 steps
    if (d.d_model != 128 && d.d_model != 384 && d.d_model != 512 && !small && !medium)
        return fail(WM_E_ARG, "d_model %d not supported (128, 384, 512, 768 or 1024)", d.d_model);
    if (small && d.ffn != 3072) return fail(WM_E_ARG, "ffn %d not supported (d_model 768 takes ffn 3072 only)", d.ffn);
    if (medium && d.ffn != 4096) return fail(WM_E_ARG, "ffn %d not supported (d_model 1024 takes ffn 4096 only)", d.ffn);
    // dec_linear_model_supports_k is what admits 3072 and 4096 (the K-long form of fc2); below d_model 768 the K-long form stays closed
    if (!dec_linear_model_supports_k(d.ffn) || (!small && !medium && d.ffn > 2048))
        return fail(WM_E_ARG, "ffn %d not supported (ffn/32 must split into <= 16 waves x <= 4 k-steps, ffn <= 2048; 3072 with d_model 768, 4096 with d_model 1024)", d.ffn);
    if ((d.n_layers * 2 * d.d_model) % 128) return fail(WM_E_ARG, "n_layers*2*d_model must be a multiple of 128");
    if (d.n_text_ctx > 512) return fail(WM_E_ARG, "n_text_ctx > 512 not supported");
    if (d.n_mels <= 0 || d.n_audio_ctx <= 0 || d.vocab <= 0 || d.n_layers <= 0) return fail(WM_E_ARG, "bad dims");
    if (c->compute_dtype < 0 || c->compute_dtype > 2) return fail(WM_E_ARG, "bad compute_dtype");
    if (!(c->kv_dtype == WM_F32 || c->kv_dtype == c->compute_dtype))
        return fail(WM_E_ARG, "kv_dtype must be WM_F32 or equal compute_dtype");
    if (c->decoder_fp32 != 0 && c->decoder_fp32 != 1) return fail(WM_E_ARG, "decoder_fp32 must be 0 or 1");
    if (c->coalesce < 0 || c->coalesce > 2) return fail(WM_E_ARG, "coalesce must be 0, 1 (both: off) or 2");
    if (c->max_batch <= 0) return fail(WM_E_ARG, "max_batch must be > 0");
    if (c->gelu_mode != 0 && c->gelu_mode != 1) return fail(WM_E_ARG, "bad gelu_mode");
    return 0;
}

// ---- model load: loader.mojo:10-27 + whisper.mojo:60-69,122-128 + layers.mojo:96-103,418-433 -------------------
struct Reader {
    const float* p;
    size_t off = 0;
    const float* take(size_t n) {
        const float* r = p + off;
        off += n;
        return r;
    }
};
struct AttnW {
    const float *q_w, *q_b, *k_w, *v_w, *v_b, *o_w, *o_b;
};
static AttnW read_attn(Reader& r, size_t d) {
    AttnW a;
    a.q_w = r.take(d * d);
    a.q_b = r.take(d);
    a.k_w = r.take(d * d);
    a.v_w = r.take(d * d);
    a.v_b = r.take(d);
    a.o_w = r.take(d * d);
    a.o_b = r.take(d);
    return a;
}
// [co][ci][3] -> [co][3][ci_pad]   (transpose_conv_weights, whisper_tensor.mojo:358-364, plus channel padding)
std::vector<float> conv_relayout(const float* w, int co, int ci, int cip) {
    std::vector<float> o((size_t)co * 3 * cip, 0.f);
    for (int a = 0; a < co; ++a)
        for (int c = 0; c < ci; ++c)
            for (int k = 0; k < 3; ++k) o[((size_t)a * 3 + k) * cip + c] = w[(size_t)a * ci * 3 + (size_t)c * 3 + k];
    return o;
}


extern "C" void wm_model_free(wm_model* m) {
    if (m && trace_events_on()) {
        trace_dump();
        {
            const char* path = wm_env("WM_TRACE_EVENTS");
            if (m->ts_buf.p && path) {
                std::vector<long long> h((2u << 20) + 1);
                if (hipMemcpy(h.data(), m->ts_buf.p, h.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
                    if (FILE* f = fopen(path, "w")) {
                        const long long n = std::min<long long>(h[0], 1ll << 20);
                        for (long long i = 0; i < n; ++i) fprintf(f, "%lld %lld %lld\n", h[1 + 2 * i] >> 8, h[1 + 2 * i] & 255, h[2 + 2 * i]);
                        fclose(f);
                    }
                }
            }
        }
    }
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->pump.joinable()) {
        {
            std::lock_guard<std::mutex> lk(m->pump_mu);
            m->pump_quit = true;
        }
        m->pump_cv.notify_all();
        m->pump.join();
    }
    // the model owns every state created on it (pipeline slots and the caller's KVCaches): a handle the caller still holds
    // becomes stale — wm_state_free / wm_decode_step on it is a checked no-op / error, not a use after free
    while (!m->states.empty()) wm_state_free(*m->states.begin());
    {
        DevBuf* fb[] = {&m->fe.window, &m->fe.dft, &m->fe.fb, &m->fe.band, &m->fe.pcm, &m->fe.lens, &m->fe.frames, &m->fe.spec, &m->fe.logtmp, &m->fe.mel};
        for (DevBuf* b : fb) b->release();
        for (auto* r : m->fe.rs) {
            r->taps.release();
            r->span.release();
            delete r;
        }
        DevBuf* lb[] = {&m->lf.pcm, &m->lf.lens, &m->lf.frames, &m->lf.spec, &m->lf.part, &m->lf.mel, &m->lf.in_mel,
                        &m->lf.win[0], &m->lf.win[1], &m->lf.items[0], &m->lf.items[1]};
        for (DevBuf* b : lb) b->release();
    }
    DevBuf* top[] = {&m->conv1_w, &m->conv1_b, &m->conv2_w, &m->conv2_b, &m->enc_pos, &m->enc_ln_g, &m->enc_ln_b,
                     &m->tok_emb_f, &m->tok_emb_t, &m->dec_pos, &m->dec_ln_g, &m->dec_ln_b, &m->cross_kv_w, &m->cross_kv_b};
    for (DevBuf* b : top) b->release();
    for (EncLayer& l : m->enc) {
        DevBuf* bs[] = {&l.qkv_w, &l.qkv_b, &l.o_w, &l.o_b, &l.ln1_g, &l.ln1_b, &l.fc1_w, &l.fc1_b, &l.fc2_w, &l.fc2_b, &l.ln2_g, &l.ln2_b};
        for (DevBuf* b : bs) b->release();
    }
    for (DecLayer& l : m->dec) {
        DevBuf* bs[] = {&l.sqkv_w, &l.sqkv_b, &l.so_w, &l.so_b, &l.ln1_g, &l.ln1_b, &l.cq_w, &l.cq_b, &l.co_w, &l.co_b,
                        &l.lnx_g, &l.lnx_b, &l.fc1_w, &l.fc1_b, &l.fc2_w, &l.fc2_b, &l.ln2_g, &l.ln2_b};
        for (DevBuf* b : bs) b->release();
    }
    if (m->stream) (void)hipStreamDestroy(m->stream);
    delete m;
}

static int model_build(wm_model* m, const float* w) {
    const wm_dims& c = m->cfg.dims;
    const size_t d = c.d_model, f = c.ffn;
    const int T = m->cfg.compute_dtype;  // encoder-side operands (incl. the cross-K/V projection of the encoder output)
    const int TD = dec_dtype(m->cfg);    // decoder-side operands
    Reader r{w};
    m->Cp = (c.n_mels + 31) / 32 * 32;
    m->Vpad = (c.vocab + 15) / 16 * 16;
    {
        // conv1 as implicit GEMM: K = 3*Cp, rounded up to a multiple of 64 with zero weights (the extra window elements
        // read the start of the next token row and are multiplied by 0) so the 16-bit path takes the LDS-staged kernel
        auto c1r = conv_relayout(r.take(d * c.n_mels * 3), c.d_model, c.n_mels, m->Cp);
        m->K1 = (3 * m->Cp + 63) / 64 * 64;
        std::vector<float> c1((size_t)c.d_model * m->K1, 0.f);
        for (int a = 0; a < c.d_model; ++a) memcpy(&c1[(size_t)a * m->K1], &c1r[(size_t)a * 3 * m->Cp], (size_t)3 * m->Cp * 4);
        WMCHK(upload(m->conv1_w, c1.data(), c1.size(), T));
        WMCHK(upload(m->conv1_b, r.take(d), d, WM_F32));
        auto c2 = conv_relayout(r.take(d * d * 3), c.d_model, c.d_model, c.d_model);
        WMCHK(upload(m->conv2_w, c2.data(), c2.size(), T));
        WMCHK(upload(m->conv2_b, r.take(d), d, WM_F32));
        WMCHK(upload(m->enc_pos, r.take((size_t)c.n_audio_ctx * d), (size_t)c.n_audio_ctx * d, WM_F32));
    }
    std::vector<float> qkv(3 * d * d), qkvb(3 * d);
    auto pack_qkv = [&](const AttnW& a) {
        memcpy(qkv.data(), a.q_w, d * d * 4);
        memcpy(qkv.data() + d * d, a.k_w, d * d * 4);
        memcpy(qkv.data() + 2 * d * d, a.v_w, d * d * 4);
        memcpy(qkvb.data(), a.q_b, d * 4);
        memset(qkvb.data() + d, 0, d * 4);  // k_proj has no bias (layers.mojo:96-103)
        memcpy(qkvb.data() + 2 * d, a.v_b, d * 4);
    };
    m->enc.resize(c.n_layers);
    for (int i = 0; i < c.n_layers; ++i) {
        EncLayer& l = m->enc[i];
        AttnW a = read_attn(r, d);
        pack_qkv(a);
        WMCHK(upload(l.qkv_w, qkv.data(), qkv.size(), T));
        WMCHK(upload(l.qkv_b, qkvb.data(), qkvb.size(), WM_F32));
        WMCHK(upload(l.o_w, a.o_w, d * d, T));
        WMCHK(upload(l.o_b, a.o_b, d, WM_F32));
        WMCHK(upload(l.ln1_g, r.take(d), d, WM_F32));
        WMCHK(upload(l.ln1_b, r.take(d), d, WM_F32));
        WMCHK(upload(l.fc1_w, r.take(f * d), f * d, T));
        WMCHK(upload(l.fc1_b, r.take(f), f, WM_F32));
        WMCHK(upload(l.fc2_w, r.take(d * f), d * f, T));
        WMCHK(upload(l.fc2_b, r.take(d), d, WM_F32));
        WMCHK(upload(l.ln2_g, r.take(d), d, WM_F32));
        WMCHK(upload(l.ln2_b, r.take(d), d, WM_F32));
    }
    WMCHK(upload(m->enc_ln_g, r.take(d), d, WM_F32));
    WMCHK(upload(m->enc_ln_b, r.take(d), d, WM_F32));
    {
        const float* te = r.take((size_t)c.vocab * d);
        WMCHK(upload(m->tok_emb_f, te, (size_t)c.vocab * d, WM_F32));
        if (TD != WM_F32) WMCHK(upload(m->tok_emb_t, te, (size_t)c.vocab * d, TD));
        WMCHK(upload(m->dec_pos, r.take((size_t)c.n_text_ctx * d), (size_t)c.n_text_ctx * d, WM_F32));
    }
    std::vector<float> ckv((size_t)c.n_layers * 2 * d * d), ckvb((size_t)c.n_layers * 2 * d, 0.f);
    m->dec.resize(c.n_layers);
    for (int i = 0; i < c.n_layers; ++i) {
        DecLayer& l = m->dec[i];
        AttnW a = read_attn(r, d);
        pack_qkv(a);
        WMCHK(upload(l.sqkv_w, qkv.data(), qkv.size(), TD));
        WMCHK(upload(l.sqkv_b, qkvb.data(), qkvb.size(), WM_F32));
        WMCHK(upload(l.so_w, a.o_w, d * d, TD));
        WMCHK(upload(l.so_b, a.o_b, d, WM_F32));
        WMCHK(upload(l.ln1_g, r.take(d), d, WM_F32));
        WMCHK(upload(l.ln1_b, r.take(d), d, WM_F32));
        AttnW x = read_attn(r, d);
        WMCHK(upload(l.cq_w, x.q_w, d * d, TD));
        WMCHK(upload(l.cq_b, x.q_b, d, WM_F32));
        memcpy(ckv.data() + (size_t)(2 * i) * d * d, x.k_w, d * d * 4);
        memcpy(ckv.data() + (size_t)(2 * i + 1) * d * d, x.v_w, d * d * 4);
        memcpy(ckvb.data() + (size_t)(2 * i + 1) * d, x.v_b, d * 4);
        WMCHK(upload(l.co_w, x.o_w, d * d, TD));
        WMCHK(upload(l.co_b, x.o_b, d, WM_F32));
        WMCHK(upload(l.lnx_g, r.take(d), d, WM_F32));
        WMCHK(upload(l.lnx_b, r.take(d), d, WM_F32));
        WMCHK(upload(l.fc1_w, r.take(f * d), f * d, TD));
        WMCHK(upload(l.fc1_b, r.take(f), f, WM_F32));
        WMCHK(upload(l.fc2_w, r.take(d * f), d * f, TD));
        WMCHK(upload(l.fc2_b, r.take(d), d, WM_F32));
        WMCHK(upload(l.ln2_g, r.take(d), d, WM_F32));
        WMCHK(upload(l.ln2_b, r.take(d), d, WM_F32));
    }
    WMCHK(upload(m->dec_ln_g, r.take(d), d, WM_F32));
    WMCHK(upload(m->dec_ln_b, r.take(d), d, WM_F32));
    WMCHK(upload(m->cross_kv_w, ckv.data(), ckv.size(), T));
    WMCHK(upload(m->cross_kv_b, ckvb.data(), ckvb.size(), WM_F32));
    if (const char* tr = wm_env("WM_TRACE_EVENTS"); tr && strchr(tr, '/')) WMCHK(m->ts_buf.alloc(((2u << 20) + 1) * 8, true));
    if (r.off != wm_synth_count(&c)) return fail(WM_E_SIZE, "internal: consumed %zu floats, expected %zu", r.off, wm_synth_count(&c));
    return 0;
}

extern "C" int wm_model_load_memory(const float* weights, size_t n_floats, const wm_config* cfg, int device, wm_model** out) {
    if (!weights || !cfg || !out) return fail(WM_E_ARG, "null argument");
    WMCHK(check_cfg(cfg));
    const size_t want = wm_synth_count(&cfg->dims);
    if (n_floats != want)
        return fail(WM_E_SIZE, "weight image holds %zu floats (%zu bytes), this config needs %zu (%zu bytes)", n_floats,
                    n_floats * 4, want, want * 4);
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(WM_E_ARG, "device %d out of range (%d visible)", device, ndev);
    HIPCHK(hipSetDevice(device));
    wm_model* m = new wm_model();
    m->cfg = *cfg;
    m->device = device;
    if (const char* e = wm_env("WM_ENC_CHUNK")) m->enc_chunk = std::max(1, atoi(e));
    m->xattn = cfg->compute_dtype == WM_BF16 && cfg->kv_dtype == WM_F32 && cfg->dims.n_heads <= 8 &&
               cfg->dims.d_model == 64 * cfg->dims.n_heads && !wm_env("WM_XATTN_OFF");
    hipError_t e = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete m;
        return fail(WM_E_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
    }
    int rc = model_build(m, weights);
    if (rc) {
        std::string keep = g_err;
        wm_model_free(m);
        g_err = keep;
        return rc;
    }
    *out = m;
    return 0;
}

// ---- weight file formats ------------------------------------------------------------------------------------------
// v1: the reference's headerless fp32 dump (export_weights.py:19-90; loader.mojo reads it with no size check).
// v2: 64-byte header {magic "WMIWGT2", version, matrix dtype, dims, flags, payload bytes} + the same
// tensors in the same order; conv / linear matrices (and, unless flag bit 0 is set, the token embedding) stored in the
// matrix dtype, every vector and positional table in fp32.  Loading v2 expands to the fp32 image the builder takes, so a
// v2 file in the model's compute dtype gives bit-identical weights to the v1 file (16-bit rounding is idempotent).
struct WmV2Header {
    char magic[8];
    uint32_t version, matrix_dtype;
    int32_t dims[8];
    uint32_t flags, reserved;
    uint64_t payload_bytes;
};
static_assert(sizeof(WmV2Header) == 64, "v2 header is 64 bytes");
static const char WM_V2_MAGIC[8] = {'W', 'M', 'I', 'W', 'G', 'T', '2', '\0'};
enum { WM_V2_EMB_F32 = 1 };

struct TensorSpan {
    int kind;
    size_t count;
};
static void collect_tensor(void* user, int, int kind, size_t count) { ((std::vector<TensorSpan>*)user)->push_back({kind, count}); }
static bool v2_is_matrix(int kind, uint32_t flags) { return kind == WM_K_WEIGHT || kind == WM_K_QK || (kind == WM_K_EMB && !(flags & WM_V2_EMB_F32)); }
static size_t v2_payload_bytes(const wm_dims* d, int dtype, uint32_t flags) {
    std::vector<TensorSpan> t;
    wm_synth_walk(d, collect_tensor, &t);
    size_t n = 0;
    for (auto& s : t) n += s.count * (v2_is_matrix(s.kind, flags) ? dt_size(dtype) : 4);
    return n;
}
static inline float bf16_to_f32_host(uint16_t h) {
    uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static inline float f16_to_f32_host(uint16_t h) {
    _Float16 x;
    memcpy(&x, &h, 2);
    return (float)x;
}

extern "C" int wm_weights_convert_v2(const char* v1_path, const char* v2_path, const wm_dims* dims, int dtype, int emb_f32) {
    if (!v1_path || !v2_path || !dims || dtype < 0 || dtype > 2) return fail(WM_E_ARG, "bad argument");
    const size_t n = wm_synth_count(dims);
    FILE* f = fopen(v1_path, "rb");
    if (!f) return fail(WM_E_IO, "cannot open %s", v1_path);
    fseek(f, 0, SEEK_END);
    const long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (sz < 0 || (size_t)sz != n * 4) {
        fclose(f);
        return fail(WM_E_SIZE, "%s is %ld bytes, these dims need %zu", v1_path, sz, n * 4);
    }
    std::vector<float> w(n);
    const size_t got = fread(w.data(), 4, n, f);
    fclose(f);
    if (got != n) return fail(WM_E_IO, "short read on %s", v1_path);
    WmV2Header h{};
    memcpy(h.magic, WM_V2_MAGIC, 8);
    h.version = 2;
    h.matrix_dtype = (uint32_t)dtype;
    memcpy(h.dims, dims, sizeof h.dims);
    h.flags = emb_f32 ? WM_V2_EMB_F32 : 0;
    h.payload_bytes = v2_payload_bytes(dims, dtype, h.flags);
    FILE* o = fopen(v2_path, "wb");
    if (!o) return fail(WM_E_IO, "cannot create %s", v2_path);
    bool ok = fwrite(&h, sizeof h, 1, o) == 1;
    std::vector<TensorSpan> t;
    wm_synth_walk(dims, collect_tensor, &t);
    size_t off = 0;
    std::vector<uint16_t> tmp;
    for (auto& s : t) {
        if (v2_is_matrix(s.kind, h.flags) && dtype != WM_F32) {
            tmp.resize(s.count);
            for (size_t i = 0; i < s.count; ++i) tmp[i] = dtype == WM_BF16 ? f32_to_bf16_host(w[off + i]) : f32_to_f16_host(w[off + i]);
            ok = ok && fwrite(tmp.data(), 2, s.count, o) == s.count;
        } else {
            ok = ok && fwrite(w.data() + off, 4, s.count, o) == s.count;
        }
        off += s.count;
    }
    ok = (fclose(o) == 0) && ok;
    return ok ? 0 : fail(WM_E_IO, "write error on %s", v2_path);
}

// Reads a v1 or v2 file into an fp32 image of wm_weight_count(dims) floats, validating size / header against dims.
extern "C" int wm_weights_read(const char* path, const wm_dims* dims, float* out) {
    if (!path || !dims || !out) return fail(WM_E_ARG, "null argument");
    const size_t n = wm_synth_count(dims);
    FILE* f = fopen(path, "rb");
    if (!f) return fail(WM_E_IO, "cannot open %s", path);
    fseek(f, 0, SEEK_END);
    const long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    WmV2Header h{};
    const bool v2 = sz >= (long)sizeof h && fread(&h, sizeof h, 1, f) == 1 && memcmp(h.magic, WM_V2_MAGIC, 8) == 0;
    if (!v2) {
        fseek(f, 0, SEEK_SET);
        if (sz < 0 || (size_t)sz != n * 4) {
            fclose(f);
            return fail(WM_E_SIZE, "%s is %ld bytes, this config needs %zu", path, sz, n * 4);
        }
        const size_t got = fread(out, 4, n, f);
        fclose(f);
        return got == n ? 0 : fail(WM_E_IO, "short read on %s", path);
    }
    int rc = 0;
    if (h.version != 2 || h.matrix_dtype > 2)
        rc = fail(WM_E_SIZE, "%s: unsupported v2 header (version %u, dtype %u)", path, h.version, h.matrix_dtype);
    else if (memcmp(h.dims, dims, sizeof h.dims) != 0)
        rc = fail(WM_E_SIZE, "%s was written for other dims (d_model %d, layers %d, vocab %d)", path, h.dims[0], h.dims[2], h.dims[7]);
    else if (h.payload_bytes != v2_payload_bytes(dims, (int)h.matrix_dtype, h.flags) || (size_t)sz != sizeof h + h.payload_bytes)
        rc = fail(WM_E_SIZE, "%s: payload size does not match its header", path);
    if (!rc) {
        std::vector<TensorSpan> t;
        wm_synth_walk(dims, collect_tensor, &t);
        size_t off = 0;
        std::vector<uint16_t> tmp;
        for (auto& s : t) {
            if (v2_is_matrix(s.kind, h.flags) && h.matrix_dtype != WM_F32) {
                tmp.resize(s.count);
                if (fread(tmp.data(), 2, s.count, f) != s.count) {
                    rc = fail(WM_E_IO, "short read on %s", path);
                    break;
                }
                for (size_t i = 0; i < s.count; ++i) out[off + i] = h.matrix_dtype == WM_BF16 ? bf16_to_f32_host(tmp[i]) : f16_to_f32_host(tmp[i]);
            } else if (fread(out + off, 4, s.count, f) != s.count) {
                rc = fail(WM_E_IO, "short read on %s", path);
                break;
            }
            off += s.count;
        }
    }
    fclose(f);
    return rc;
}

extern "C" int wm_model_load(const char* path, const wm_config* cfg, int device, wm_model** out) {
    if (!path || !cfg || !out) return fail(WM_E_ARG, "null argument");
    WMCHK(check_cfg(cfg));
    std::vector<float> buf(wm_synth_count(&cfg->dims));
    WMCHK(wm_weights_read(path, &cfg->dims, buf.data()));
    return wm_model_load_memory(buf.data(), buf.size(), cfg, device, out);
}

// ---- state ---------------------------------------------------------------------------------------------------
extern "C" void wm_state_free(wm_state* s) {
    if (!s) return;
    {
        std::lock_guard<std::mutex> lk(g_states_mu);
        if (!g_live_states.erase(s)) return;  // stale handle: its model was freed (and took the state with it)
    }
    {  // the loop pump must not touch this state any more (it works under this mutex)
        std::lock_guard<std::mutex> lk(s->m->pump_mu);
        auto& wq = s->m->pump_work;
        wq.erase(std::remove(wq.begin(), wq.end(), s), wq.end());
    }
    s->m->states.erase(s);
    if (s->m->cached == s) s->m->cached = nullptr;
    for (auto& sl : s->m->slots)
        if (sl == s) sl = nullptr;
    for (auto& pr : s->m->pairs)
        if (pr == s) pr = nullptr;
    for (auto& ls : s->m->lf.st)
        if (ls == s) ls = nullptr;
    for (auto& r : s->m->slot_ref)
        if (r.st == s) r = wm_model::SlotRef{};
    for (auto& r : s->m->align_ref)
        if (r.st == s) r = wm_model::AlignRef{};
    for (auto& r : s->m->topk_ref)
        if (r.st == s) r = wm_model::TopkRef{};
    for (auto& r : s->m->ct_ref)
        if (r.st == s) r = wm_model::ConstraintRef{};
    (void)hipSetDevice(s->m->device);
    // nothing of this state may still be running when its graphs, streams and arenas go away (a submitted pass that was
    // never waited for, or the model stream's last wm_decode_step)
    for (auto& ln : s->lanes)
        if (ln.st) (void)hipStreamSynchronize(ln.st);
    if (s->m->stream) (void)hipStreamSynchronize(s->m->stream);
    for (auto& ln : s->lanes) {
        for (auto& g : ln.graph)
            if (g) (void)hipGraphExecDestroy(g);
        if (ln.st) (void)hipStreamDestroy(ln.st);
        if (ln.done) (void)hipEventDestroy(ln.done);
    }
    if (s->enc_done) (void)hipEventDestroy(s->enc_done);
    for (auto& ev : s->sc.ev)
        if (ev) (void)hipEventDestroy(ev);
    for (auto& ev : s->chunk_ev)
        if (ev) (void)hipEventDestroy(ev);
    if (s->h_prog) (void)hipHostFree((void*)s->h_prog);
    DevBuf* bs[] = {&s->mel_dev, &s->mel_t, &s->h1, &s->x, &s->xn, &s->qkv, &s->ao, &s->hid, &s->enc_t, &s->enc_f,
                    &s->cross_kv, &s->enc_x, &s->xq, &s->part_y, &s->self_kv, &s->dx, &s->dq, &s->dattn, &s->dhid, &s->part_o, &s->part_ml, &s->logits, &s->amax_val, &s->amax_idx, &s->ts_state, &s->ts_val, &s->ts_idx, &s->ts_m, &s->ts_s, &s->mask_steady, &s->mask_begin,
                    &s->tok, &s->pos, &s->tok_rows, &s->pos_rows, &s->ctl, &s->out_tokens, &s->n_tokens, &s->finished,
                    &s->al.cap, &s->al.kh, &s->al.probs, &s->al.mean, &s->al.stdv, &s->al.M, &s->al.trace, &s->al.times, &s->al.ncols,
                    &s->al.rows, &s->al.row0, &s->al.map, &s->sc.rows, &s->sc.a, &s->sc.pmax, &s->sc.psum, &s->sc.pidx, &s->sc.ztgt, &s->sc.target,
                    &s->sc.slot, &s->sc.dst, &s->sc.len, &s->sc.ctx, &s->sc.lp, &s->sc.top, &s->sc.sum, &s->sc.avg,
                    &s->rw.table, &s->rw.len, &s->rw.key_lo, &s->lp.part_s, &s->lp.table, &s->lp.sum, &s->tk.rows, &s->tk.ids, &s->tk.lps,
                    &s->ns.x, &s->ns.pmax, &s->ns.pidx, &s->ns.psum, &s->ns.prob, &s->ns.lse,
                    &s->lg.x, &s->lg.ids, &s->lg.col, &s->lg.out, &s->lg.probs, &s->rp.seen, &s->rp.ban, &s->rp.ctl, &s->rp.hit, &s->rp.val, &s->rp.sbctl,
                    &s->rp.node, &s->rp.match, &s->rp.ctctl};
    for (DevBuf* b : bs) b->release();
    delete s;
}

static const int OUT_STRIDE_MAX = 1024;

// decode lanes a state of B utterances gets (1 unless the developer build's WM_DEC_LANES asks for more)
int dec_lanes_for(int B) {
    int nl = 1;
    if (const char* e = wm_env("WM_DEC_LANES")) nl = std::max(1, std::min(4, atoi(e)));
    return std::min(nl, (B + 15) / 16);
}
// pair: the 2·B-row state of a coalesced pair of submits (B <= max_batch each)
static int state_new(wm_model* m, int B, wm_state** out, bool pair) {
    if (!m || !out || B <= 0) return fail(WM_E_ARG, "bad argument");
    if (B > m->cfg.max_batch * (pair ? 2 : 1)) return fail(WM_E_ARG, "batch %d exceeds max_batch %d", B, m->cfg.max_batch);
    HIPCHK(hipSetDevice(m->device));
    const wm_dims& c = m->cfg.dims;
    const size_t d = c.d_model, L = 2 * (size_t)c.n_audio_ctx, T = c.n_audio_ctx;
    const size_t ts = dt_size(m->cfg.compute_dtype), ks = dt_size(m->cfg.kv_dtype);
    wm_state* s = new wm_state();
    s->m = m;
    s->B = B;
    {
        std::lock_guard<std::mutex> lk(g_states_mu);
        g_live_states.insert(s);
    }
    m->states.insert(s);
    s->Bc = std::min(pair ? B / 2 : B, m->enc_chunk);  // (pair: an encoder chunk never straddles the two batches)
    // key chunks per utterance for the cross-attention kernel: a function of the MODEL's max_batch, never of this call's
    // B, so that an utterance's result does not depend on how it was batched (bitwise batch invariance within a model).
    // Aim for 1024 workgroups at full batch (4 per CU, one full round): 16 chunks at max_batch 64 (measured, µs per launch /
    // per whole step: 12 chunks 26.4 / 280, 16: 25.2 / 273, 20: 25.5 / 278, 24: 26.4 / 278), up to 48 for small-batch /
    // latency models (B = 1: 12.1 -> 4 us per launch).  WM_NSPLIT overrides for tuning.
    {
        const int min_split = (int)((T + 511) / 512);
        // fp32 K/V rows are twice as wide: half the chunks move the same bytes per workgroup, the stream runs as fast (46.6 vs 46.5 us
        // per launch at B = 64) and the merge reads half the partials (decode step 406 -> 402 us; 10 / 12 chunks: 418 / 412 us)
        const int target = ks == 4 ? 512 : 1024;
        int ns = (target + m->cfg.max_batch - 1) / m->cfg.max_batch;
        ns = std::max(ks == 4 ? 8 : 12, std::min(48, ns));
        ns = std::max(min_split, std::min(ns, (int)((T + 31) / 32)));
        if (m->xattn) {
            // absorbed cross-attention: a chunk carries fixed costs the K/V stream did not have (q' images into LDS, an H·d partial,
            // its share of the merge), so fewer, longer chunks: ~128 per max_batch rows, at least 64 keys (one tile per wave).
            // Measured, headline (128-row states), ms per 64-clip pass: 32 chunks 32.1, 24: 28.3, 16: 26.0, 8: 23.5, 6: 23.5,
            // 4: 22.3-22.5, 3: 21.8, 2: 21.4
            ns = (128 + m->cfg.max_batch - 1) / m->cfg.max_batch;
            ns = std::max(1, std::min({ns, 48, (int)T / 64}));
        }
        if (const char* e = wm_env("WM_NSPLIT")) ns = std::max(m->xattn ? 1 : min_split, std::min(64, atoi(e)));
        s->nsplit = ns;
    }
    s->out_stride = OUT_STRIDE_MAX;
    const size_t Bc = s->Bc;
    const size_t Mp = (Bc * T + 255) / 256 * 256 + 256;  // padded rows: tail tiles (up to 256 rows) read, never store, past M
    int rc = 0;
    auto A = [&](DevBuf& b, size_t bytes, bool zero = false) {
        if (!rc) rc = b.alloc(bytes, zero);
    };
    A(s->mel_dev, (size_t)B * c.n_mels * L * 4);
    A(s->mel_t, (Bc * (L + 2) + 256) * m->Cp * ts, true);
    A(s->h1, (Bc * (L + 2) + 256) * d * ts, true);  // rows 0 and L+1 of each utterance stay zero = conv padding
    A(s->x, Mp * d * 4, true);
    A(s->xn, Mp * d * ts, true);
    A(s->qkv, Mp * 3 * d * ts, true);
    A(s->ao, Mp * d * ts, true);
    A(s->hid, Mp * c.ffn * ts, true);
    A(s->enc_f, (size_t)B * T * d * 4);
    if (m->xattn) {  // X rows are written in place by the encoder's last LayerNorm: no chunk-sized operand buffer, no cross cache
        A(s->enc_x, (size_t)B * T * d * 2);
    } else {
        A(s->enc_t, Mp * d * ts, true);
        A(s->cross_kv, (size_t)c.n_layers * 2 * B * T * d * ks);
    }
    A(s->self_kv, (size_t)c.n_layers * 2 * B * c.n_text_ctx * d * ks, true);
    // decode activations: rows for one token per utterance, or — prompt prefill — for up to PREFILL_MAX positions at once
    const size_t R = (size_t)B * wm_state::PREFILL_MAX;
    A(s->dx, R * d * 4);
    A(s->dq, R * d * 4);
    A(s->dattn, R * d * 4);
    A(s->dhid, R * c.ffn * 4);
    if (m->xattn) {
        A(s->xq, R * 3 * c.n_heads * d * 2);
        A(s->part_y, R * s->nsplit * c.n_heads * d * 4);
    } else {
        A(s->part_o, R * s->nsplit * d * 4);
    }
    A(s->part_ml, R * s->nsplit * c.n_heads * 2 * 4);
    A(s->tok_rows, R * 4, true);
    A(s->pos_rows, R * 4, true);
    A(s->logits, (size_t)B * m->Vpad * 4);
    s->npart = dec_logits_parts(c.vocab);
    A(s->amax_val, (size_t)B * s->npart * 4);
    A(s->amax_idx, (size_t)B * s->npart * 4);
    A(s->ts_val, (size_t)B * s->npart * 4, true);
    A(s->ts_idx, (size_t)B * s->npart * 4, true);
    A(s->ts_m, (size_t)B * s->npart * 4, true);
    A(s->ts_s, (size_t)B * s->npart * 4, true);
    A(s->ts_state, (size_t)B * sizeof(TsState), true);
    A(s->mask_steady, (size_t)m->Vpad * 4, true);
    A(s->mask_begin, (size_t)m->Vpad * 4, true);
    A(s->tok, (size_t)B * 4, true);
    A(s->pos, (size_t)B * 4, true);
    A(s->ctl, sizeof(StepCtl) * 8, true);  // [0] whole-batch control (wm_decode_step), [1..] one per decode lane
    A(s->out_tokens, (size_t)B * s->out_stride * 4, true);
    A(s->n_tokens, (size_t)B * 4, true);
    A(s->finished, (size_t)B * 4, true);
    A(s->lp.part_s, (size_t)B * s->npart * 4, true);
    A(s->lp.table, (size_t)B * s->out_stride * 4, true);
    A(s->lp.sum, (size_t)B * 4, true);
    A(s->tk.rows, (size_t)B * sizeof(TopkRow), true);
    A(s->tk.ids, (size_t)B * s->out_stride * TOPK_MAX * 4, true);
    A(s->tk.lps, (size_t)B * s->out_stride * TOPK_MAX * 4, true);
    A(s->ns.x, (size_t)B * d * 4, true);
    A(s->ns.pmax, (size_t)B * s->npart * 4, true);
    A(s->ns.pidx, (size_t)B * s->npart * 4, true);
    A(s->ns.psum, (size_t)B * s->npart * 4, true);
    A(s->ns.prob, (size_t)B * 4, true);
    A(s->ns.lse, (size_t)B * 4, true);
    A(s->lg.x, (size_t)B * d * 4, true);
    A(s->lg.ids, (size_t)LANG_DETECT_MAX * 4, true);
    A(s->lg.col, (size_t)B * 4, true);
    A(s->lg.out, (size_t)B * 4, true);
    A(s->lg.probs, (size_t)B * LANG_DETECT_MAX * 4, true);
    if (rc) {
        std::string keep = g_err;
        wm_state_free(s);
        g_err = keep;
        return rc;
    }
    {  // decode lanes
        // measured on MI355X (round 1): 2 lanes 49.1 ms vs 1 lane 47.4 ms per 64-clip pass — kernel boundaries of one
        // queue also stall the other queue's kernels, so extra lanes stay opt-in (WM_DEC_LANES)
        const int nl = dec_lanes_for(B);
        s->lanes.resize(nl);
        const int per = ((B + nl - 1) / nl + 15) / 16 * 16;  // whole MFMA row blocks per lane
        int b0 = 0;
        for (int i = 0; i < nl; ++i) {
            wm_state::Lane& ln = s->lanes[i];
            ln.b0 = b0;
            ln.nb = std::max(0, std::min(per, B - b0));
            b0 += ln.nb;
            ln.ctl = s->ctl.as<StepCtl>() + 1 + i;
            // decode launches are latency-critical (34 dependent sub-5-us kernels per token); the encoder stream carries
            // throughput work.  WM_DEC_PRIORITY=1 puts the lane streams on the highest HIP stream priority.
            int lo_p = 0, hi_p = 0;
            (void)hipDeviceGetStreamPriorityRange(&lo_p, &hi_p);
            static const bool prio = wm_env("WM_DEC_PRIORITY") != nullptr;
            hipError_t e = prio ? hipStreamCreateWithPriority(&ln.st, hipStreamNonBlocking, hi_p)
                                : hipStreamCreateWithFlags(&ln.st, hipStreamNonBlocking);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&ln.done, hipEventDisableTiming);
            if (e != hipSuccess) {
                wm_state_free(s);
                return fail(WM_E_HIP, "lane stream: %s", hipGetErrorString(e));
            }
        }
        while (!s->lanes.empty() && s->lanes.back().nb == 0) {
            (void)hipStreamDestroy(s->lanes.back().st);
            (void)hipEventDestroy(s->lanes.back().done);
            s->lanes.pop_back();
        }
        hipError_t e = hipEventCreateWithFlags(&s->enc_done, hipEventDisableTiming);
        if (e == hipSuccess) e = hipHostMalloc((void**)&s->h_prog, 64, hipHostMallocMapped);
        if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&s->d_prog, (void*)s->h_prog, 0);
        for (auto& ev : s->chunk_ev)
            if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e != hipSuccess) {
            wm_state_free(s);
            return fail(WM_E_HIP, "event: %s", hipGetErrorString(e));
        }
    }
    *out = s;
    return 0;
}
extern "C" int wm_state_new(wm_model* m, int B, wm_state** out) { return state_new(m, B, out, false); }

extern "C" int wm_state_reset(wm_state* s) {
    if (!state_is_live(s)) return fail(WM_E_ARG, "null or stale state handle");
    HIPCHK(hipSetDevice(s->m->device));
    hipStream_t st = s->m->stream;
    HIPCHK(hipMemsetAsync(s->ctl.p, 0, s->ctl.bytes, st));
    HIPCHK(hipMemsetAsync(s->n_tokens.p, 0, s->n_tokens.bytes, st));
    HIPCHK(hipMemsetAsync(s->finished.p, 0, s->finished.bytes, st));
    s->has_enc = s->has_cross = false;
    s->host_len = 0;
    return 0;
}
extern "C" int wm_state_len(const wm_state* s) { return state_is_live(s) ? s->host_len : -1; }

// ---- encoder: whisper.mojo:71-99 ------------------------------------------------------------------------------------
static void* off_bytes(const DevBuf& b, size_t bytes) { return (char*)b.p + bytes; }

static int cross_kv_chunk(wm_model* m, wm_state* s, int c0, int bc, hipStream_t st) {
    // cross K/V for utterances [c0, c0+bc) from enc_t (rows 0..bc*T): layers.mojo:150-154, all layers in one GEMM
    const wm_dims& c = m->cfg.dims;
    const size_t d = c.d_model, T = c.n_audio_ctx;
    GemmParams p{};
    p.A = s->enc_t.p;
    p.W = m->cross_kv_w.p;
    p.C = off_bytes(s->cross_kv, (size_t)c0 * T * d * dt_size(m->cfg.kv_dtype));
    p.M = (int)(bc * T);
    p.N = c.n_layers * 2 * c.d_model;
    p.K = c.d_model;
    p.lda = d;
    p.ldw = d;
    p.ldc = d;
    p.bias = m->cross_kv_b.as<float>();
    p.group_n = c.d_model;
    p.group_stride = (long)((size_t)s->B * T * d);
    return gemm_dispatch(m->cfg.compute_dtype, m->cfg.kv_dtype, p, 1, st);
}

// mel2 / split_at (coalesced pairs): utterances [split_at, B) come from mel2 (their own batch's buffer); split_at is a multiple of Bc
// want_f32: also produce the fp32 encoder output (s->enc_f, what wm_encode returns).  The decoder never reads it — the cross-K/V
// projection consumes the operand-dtype rows s->enc_t — so the transcribe paths skip it, and where the last fc2 can carry a
// LayerNorm in its epilogue (16-bit operands, d = 384) `ln_post` rides there: no LayerNorm launch, no 147 MB fp32 write per pass.
// BOTH kinds of caller take the operand rows from the same epilogue, so wm_encode + wm_decode_step and wm_transcribe see
// bit-identical cross-K/V (round 2 had fused it for the transcribe paths only and reverted: the two entry points parted at a near-tie).
int run_encoder(wm_model* m, wm_state* s, const float* mel_dev, int B, hipStream_t st, const float* mel2, int split_at,
                       bool want_f32) {
    const wm_dims& c = m->cfg.dims;
    const int T = m->cfg.compute_dtype;
    const size_t d = c.d_model, L = 2 * (size_t)c.n_audio_ctx, NT = c.n_audio_ctx, ts = dt_size(T);
    for (int c0 = 0; c0 < B; c0 += s->Bc) {
        const int bc = std::min(s->Bc, B - c0);
        const int M = (int)(bc * NT);
        const int opb = T == WM_F32 ? 4 : 2;
        bool xn_is_ln1 = false;  // xn holds LN1(x) of the coming block, written by the epilogue of the GEMM that produced x
        bool post_fused = false;  // enc_t was written by the last fc2's epilogue
        // operand rows of ln_post: the chunk-sized enc_t that the cross-K/V projection consumes, or (m->xattn) this chunk's rows
        // of the state's X, which the decoder's cross-attention streams itself
        void* post_rows = m->xattn ? off_bytes(s->enc_x, (size_t)c0 * NT * d * 2) : s->enc_t.p;
        const float* mel_c = (mel2 && c0 >= split_at) ? mel2 + (size_t)(c0 - split_at) * c.n_mels * L : mel_dev + (size_t)c0 * c.n_mels * L;
        DISPATCH_DT(T, TT, launch_mel_transpose_pad<TT>(mel_c, s->mel_t.p, bc, c.n_mels, (int)L, m->Cp, st));
        {  // conv1 + GELU -> h1 rows 1..L (token-major)   whisper.mojo:73-75
            GemmParams p{};
            p.A = s->mel_t.p;
            p.W = m->conv1_w.p;
            p.C = off_bytes(s->h1, d * ts);
            p.M = (int)L;
            p.N = c.d_model;
            p.K = m->K1;
            p.lda = m->Cp;
            p.ldw = m->K1;
            p.ldc = d;
            p.strideA = (long)((L + 2) * m->Cp);
            p.strideC = (long)((L + 2) * d);
            p.bias = m->conv1_b.as<float>();
            p.act = 1;
            p.gelu_mode = m->cfg.gelu_mode;
            WMCHK(gemm_dispatch(T, T, p, bc, st));
        }
        {  // conv2 (stride 2) + GELU + pos_emb -> x   whisper.mojo:78-89
            GemmParams p{};
            p.A = s->h1.p;
            p.W = m->conv2_w.p;
            p.C = s->x.p;
            p.M = (int)NT;
            p.N = c.d_model;
            p.K = 3 * c.d_model;
            p.lda = 2 * d;
            p.ldw = 3 * d;
            p.ldc = d;
            p.strideA = (long)((L + 2) * d);
            p.strideC = (long)(NT * d);
            p.bias = m->conv2_b.as<float>();
            p.act = 1;
            p.gelu_mode = m->cfg.gelu_mode;
            p.pos = m->enc_pos.as<float>();
            if (gemm_nt_fuses_layernorm_out(opb, p)) {  // the first block's LN1 rides conv2's epilogue
                p.lno_g = m->enc[0].ln1_g.as<float>();
                p.lno_b = m->enc[0].ln1_b.as<float>();
                p.lno_out = s->xn.p;
                xn_is_ln1 = true;
            }
            WMCHK(gemm_dispatch(T, WM_F32, p, bc, st));
        }
        for (int l = 0; l < c.n_layers; ++l) {  // layers.mojo:435-519 with is_decoder=False
            EncLayer& w = m->enc[l];
            GemmParams p{};
            p.A = s->xn.p;
            p.W = w.qkv_w.p;
            p.C = s->qkv.p;
            p.M = M;
            p.N = 3 * c.d_model;
            p.K = c.d_model;
            p.lda = d;
            p.ldw = d;
            p.ldc = 3 * d;
            p.bias = w.qkv_b.as<float>();
            if (xn_is_ln1)  // the producer of x wrote LN1(x) next to it
                WMCHK(gemm_dispatch(T, T, p, 1, st));
            else
                WMCHK(ln_then_gemm(T, T, p, s->x.as<float>(), w.ln1_g.as<float>(), w.ln1_b.as<float>(), st));
            DISPATCH_DT(T, TT, launch_flash_attn_enc<TT>(s->qkv.p, s->ao.p, bc, c.n_heads, c.n_audio_ctx, ATTN_SCALE, st));
            GemmParams o{};
            o.A = s->ao.p;
            o.W = w.o_w.p;
            o.C = s->x.p;
            o.M = M;
            o.N = c.d_model;
            o.K = c.d_model;
            o.lda = d;
            o.ldw = d;
            o.ldc = d;
            o.bias = w.o_b.as<float>();
            o.residual = s->x.as<float>();
            o.ldr = d;
            const bool xn_is_ln2 = gemm_nt_fuses_layernorm_out(opb, o);
            if (xn_is_ln2) {
                o.lno_g = w.ln2_g.as<float>();
                o.lno_b = w.ln2_b.as<float>();
                o.lno_out = s->xn.p;
            }
            WMCHK(gemm_dispatch(T, WM_F32, o, 1, st));
            GemmParams f1{};
            f1.A = s->xn.p;
            f1.W = w.fc1_w.p;
            f1.C = s->hid.p;
            f1.M = M;
            f1.N = c.ffn;
            f1.K = c.d_model;
            f1.lda = d;
            f1.ldw = d;
            f1.ldc = c.ffn;
            f1.bias = w.fc1_b.as<float>();
            f1.act = 1;
            f1.gelu_mode = m->cfg.gelu_mode;
            if (xn_is_ln2)
                WMCHK(gemm_dispatch(T, T, f1, 1, st));
            else
                WMCHK(ln_then_gemm(T, T, f1, s->x.as<float>(), w.ln2_g.as<float>(), w.ln2_b.as<float>(), st));
            GemmParams f2{};
            f2.A = s->hid.p;
            f2.W = w.fc2_w.p;
            f2.C = s->x.p;
            f2.M = M;
            f2.N = c.d_model;
            f2.K = c.ffn;
            f2.lda = c.ffn;
            f2.ldw = c.ffn;
            f2.ldc = d;
            f2.bias = w.fc2_b.as<float>();
            f2.residual = s->x.as<float>();
            f2.ldr = d;
            const bool fuse_out = gemm_nt_fuses_layernorm_out(opb, f2);
            xn_is_ln1 = l + 1 < c.n_layers && fuse_out;
            if (xn_is_ln1) {  // the next block's LN1
                f2.lno_g = m->enc[l + 1].ln1_g.as<float>();
                f2.lno_b = m->enc[l + 1].ln1_b.as<float>();
                f2.lno_out = s->xn.p;
            } else if (fuse_out) {  // last block: ln_post (whisper.mojo:97-98) as operand rows for the cross-K/V projection
                f2.lno_g = m->enc_ln_g.as<float>();
                f2.lno_b = m->enc_ln_b.as<float>();
                f2.lno_out = post_rows;
                post_fused = true;
            }
            WMCHK(gemm_dispatch(T, WM_F32, f2, 1, st));
        }
        float* encf = s->enc_f.as<float>() + (size_t)c0 * NT * d;
        if (!post_fused)  // operand rows (and the fp32 copy) from the LayerNorm kernel
            DISPATCH_DT(T, TT, launch_layernorm_rows<TT>(s->x.as<float>(), m->enc_ln_g.as<float>(), m->enc_ln_b.as<float>(), post_rows, want_f32 ? encf : nullptr, M, c.d_model, 1e-5f, st));
        else if (want_f32)  // the fp32 copy only
            DISPATCH_DT(T, TT, launch_layernorm_rows<TT>(s->x.as<float>(), m->enc_ln_g.as<float>(), m->enc_ln_b.as<float>(), nullptr, encf, M, c.d_model, 1e-5f, st));
        if (!m->xattn) WMCHK(cross_kv_chunk(m, s, c0, bc, st));
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// B < 0: any batch size (the caller takes it from the state AFTER this check — a stale handle is never dereferenced)
int check_state(wm_model* m, wm_state* s, int B) {
    if (!m || !s) return fail(WM_E_ARG, "null handle");
    if (!state_is_live(s)) return fail(WM_E_ARG, "stale state handle (its model was freed or reloaded)");
    if (s->m != m) return fail(WM_E_ARG, "state belongs to another model");
    if (B >= 0 && B != s->B) return fail(WM_E_ARG, "B=%d but the state was created for %d", B, s->B);
    return 0;
}

extern "C" int wm_encode(wm_model* m, wm_state* s, const float* mel, int mel_on_device, int B, float* enc_out) {
    WMCHK(check_state(m, s, B));
    if (!mel) return fail(WM_E_ARG, "null mel");
    HIPCHK(hipSetDevice(m->device));
    WMCHK(wm_state_reset(s));
    const wm_dims& c = m->cfg.dims;
    const float* mel_dev = mel;
    if (!mel_on_device) {
        HIPCHK(hipMemcpyAsync(s->mel_dev.p, mel, (size_t)B * c.n_mels * 2 * c.n_audio_ctx * 4, hipMemcpyHostToDevice, m->stream));
        mel_dev = s->mel_dev.as<float>();
    }
    WMCHK(run_encoder(m, s, mel_dev, B, m->stream, nullptr, 0, enc_out != nullptr));
    s->has_enc = s->has_cross = true;
    s->last_mel = mel_dev;
    if (enc_out) HIPCHK(hipMemcpyAsync(enc_out, s->enc_f.p, (size_t)B * c.n_audio_ctx * c.d_model * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return 0;
}

extern "C" int wm_state_set_encoder_output(wm_model* m, wm_state* s, const float* enc_out, int B) {
    WMCHK(check_state(m, s, B));
    if (!enc_out) return fail(WM_E_ARG, "null enc_out");
    HIPCHK(hipSetDevice(m->device));
    WMCHK(wm_state_reset(s));
    const wm_dims& c = m->cfg.dims;
    const size_t NT = c.n_audio_ctx, d = c.d_model;
    HIPCHK(hipMemcpyAsync(s->enc_f.p, enc_out, (size_t)B * NT * d * 4, hipMemcpyHostToDevice, m->stream));
    for (int c0 = 0; c0 < B; c0 += s->Bc) {
        const int bc = std::min(s->Bc, B - c0);
        if (m->xattn) {  // the cross-attention reads the bf16 rows themselves
            launch_convert<bf16>(s->enc_f.as<float>() + (size_t)c0 * NT * d, off_bytes(s->enc_x, (size_t)c0 * NT * d * 2), (size_t)bc * NT * d, m->stream);
            continue;
        }
        DISPATCH_DT(m->cfg.compute_dtype, TT, launch_convert<TT>(s->enc_f.as<float>() + (size_t)c0 * NT * d, s->enc_t.p, (size_t)bc * NT * d, m->stream));
        WMCHK(cross_kv_chunk(m, s, c0, bc, m->stream));
    }
    HIPCHK(hipStreamSynchronize(m->stream));
    s->has_enc = s->has_cross = true;
    return 0;
}

// ---- one decode step for all B utterances: whisper.mojo:130-167 with L_tgt = 1 ------------------------------------
int dec_linear_dispatch(int dt, const DecLinearParams& p, hipStream_t st) {
    int rc = 0;
    DISPATCH_DT(dt, TT, rc = launch_dec_linear<TT>(p, st));
    return launch_rc(rc);
}
int attn_decode_dispatch(int dt, const AttnDecParams& p, hipStream_t st, const int* key_lo, const int* utt_of) {
    int rc = 0;
    DISPATCH_DT(dt, TT, rc = launch_attn_decode<TT>(p, st, key_lo, utt_of));
    return launch_rc(rc);
}

template <typename T> static T* lane_ptr(const DevBuf& buf, const DecView& v, size_t stride) { return buf.as<T>() + (size_t)v.b0 * stride; }  // view v's rows

VocabHead vocab_head(const wm_model* m) {
    return VocabHead{m->dec_ln_g.as<float>(), m->dec_ln_b.as<float>(), dec_dtype(m->cfg) == WM_F32 ? m->tok_emb_f.p : m->tok_emb_t.p,
                     m->cfg.dims.vocab, m->cfg.dims.d_model};
}

// m->xattn: the cross-attention of layer l over X for the rows of view v (P positions each): absorb + X sweep (launch_cross_attn),
// then merge + V-apply into out (cross_attn_merge).  Rows are position-major as everywhere in decode_core.
static XAttnParams xattn_params(wm_model* m, wm_state* s, int l, const DecView& v, int P) {
    const wm_dims& c = m->cfg.dims;
    const size_t d = c.d_model;
    XAttnParams x{};
    x.q = lane_ptr<float>(s->dq, v, d);
    x.Wk = off_bytes(m->cross_kv_w, (size_t)(2 * l) * d * d * 2);
    x.Wv = off_bytes(m->cross_kv_w, (size_t)(2 * l + 1) * d * d * 2);
    x.bv = m->cross_kv_b.as<float>() + (size_t)(2 * l + 1) * d;
    x.X = off_bytes(s->enc_x, (size_t)v.b0 * c.n_audio_ctx * d * 2);
    x.x_stride = (long)((size_t)c.n_audio_ctx * d);
    x.n_keys = c.n_audio_ctx;
    x.nsplit = s->nsplit;
    x.H = c.n_heads;
    x.d = c.d_model;
    x.rows = v.nb * P;
    x.q_B = P > 1 ? v.nb : 0;
    x.scale = ATTN_SCALE;
    x.qs = off_bytes(s->xq, (size_t)v.b0 * 3 * c.n_heads * d * 2);
    x.part_y = lane_ptr<float>(s->part_y, v, s->nsplit * c.n_heads * d);
    x.part_ml = lane_ptr<float>(s->part_ml, v, (size_t)s->nsplit * c.n_heads * 2);
    return x;
}
int cross_attn_merge(wm_model* m, wm_state* s, int l, const DecView& v, int P, void* out, int out_dtype) {
    XAttnParams x = xattn_params(m, s, l, v, P);
    x.out = out;
    x.out_dtype = out_dtype;
    return launch_rc(launch_xattn_merge(x, v.st));
}

int launch_cross_attn(wm_model* m, wm_state* s, int l, const DecView& v, int P) {
    // an n-best score pass (single lane: v.b0 == 0): the row in slot b reads the X or K/V of clip utt_of[b]
    const int* utt_of = s->nb.on ? s->nb.utt_of.as<int>() : nullptr;
    if (m->xattn) {
        const XAttnParams x = xattn_params(m, s, l, v, P);
        WMCHK(launch_rc(launch_xattn_absorb(x, v.st)));
        return launch_rc(launch_xattn(x, v.st, utt_of));
    }
    const wm_dims& c = m->cfg.dims;
    const size_t d = c.d_model, ks = dt_size(m->cfg.kv_dtype);
    const size_t cross_l = (size_t)s->B * c.n_audio_ctx * d;
    const size_t boff = (size_t)v.b0 * c.n_audio_ctx * d;
    AttnDecParams a{};
    a.q = lane_ptr<float>(s->dq, v, d);
    a.K = off_bytes(s->cross_kv, ((size_t)(2 * l) * cross_l + boff) * ks);
    a.V = off_bytes(s->cross_kv, ((size_t)(2 * l + 1) * cross_l + boff) * ks);
    a.batch_stride = (long)((size_t)c.n_audio_ctx * d);
    a.n_keys = c.n_audio_ctx;
    a.ctl = v.ctl;
    a.nsplit = s->nsplit;
    a.scale = ATTN_SCALE;
    a.part_o = lane_ptr<float>(s->part_o, v, s->nsplit * d);
    a.part_ml = lane_ptr<float>(s->part_ml, v, (size_t)s->nsplit * c.n_heads * 2);
    a.H = c.n_heads;
    a.d = c.d_model;
    a.B = v.nb * P;
    a.q_B = P > 1 ? v.nb : 0;
    static const bool no_mq = wm_env("WM_NO_MQ_PREFILL") != nullptr;
    a.nq = (P == 4 && !no_mq) ? 4 : 0;  // the reference's 4-token prompt: one K/V sweep for the four positions
    a.ts = (long long*)m->ts_buf.p;
    a.ts_id = s->trace_id;
    // fewer K/V-streaming workgroups per CU when passes share the chip (AttnDecParams.lds_pad).  16-bit K/V: 34 KB of pad (+ 20 KB
    // static) = two per CU.  fp32 K/V (12 KB static): ONE per CU measured best with four 128-row passes in flight — pipelined ms per
    // 64-clip pass: pad 0 (four per CU) 28.2, 20 KB 28.4, 34 KB (three) 27.8, 42 / 50 / 60 KB (two) 27.3 / 27.5 / 27.4, 90 KB (one) 27.05
    a.lds_pad = s->shares_chip ? (m->cfg.kv_dtype == WM_F32 ? 90000 : 34 * 1024) : 0;
    return attn_decode_dispatch(m->cfg.kv_dtype, a, v.st, nullptr, utt_of);
}

// What every linear launch of a decoder pass sets (ln_g null: no LayerNorm prologue); each block's special part is added by name below
DecLinearParams linear_block(const float* x, const float* ln_g, const float* ln_b, const void* W, const float* bias, int N, int K, int B,
                             float* out, int ldo) {
    DecLinearParams p{};
    p.x = x;
    p.ldx = K;
    p.ln_g = ln_g;
    p.ln_b = ln_b;
    p.W = W;
    p.N = N;
    p.K = K;
    p.B = B;
    p.bias = bias;
    p.out = out;
    p.ldo = ldo;
    return p;
}
static void* self_kv_rows(wm_model* m, wm_state* s, const DecView& v, int l, int k_or_v) {  // layer l's cached K (0) / V (1) rows of view v
    const size_t per_utt = (size_t)m->cfg.dims.n_text_ctx * m->cfg.dims.d_model;
    return off_bytes(s->self_kv, ((size_t)(2 * l + k_or_v) * s->B + v.b0) * per_utt * dt_size(m->cfg.kv_dtype));
}
static void add_cache_append(DecLinearParams& p, wm_model* m, wm_state* s, const DecView& v, int l, int P) {  // k, v to cache row len (+ t)
    const wm_dims& c = m->cfg.dims;
    p.kcache = self_kv_rows(m, s, v, l, 0);
    p.vcache = self_kv_rows(m, s, v, l, 1);
    p.kv_batch_stride = (long)((size_t)c.n_text_ctx * c.d_model);
    p.d_model = c.d_model;
    p.kv_dtype = m->cfg.kv_dtype;
    p.kv_B = P > 1 ? v.nb : 0;
    p.ctl = v.ctl;
}
static void add_align_capture(DecLinearParams& p, const wm_state::Align& al, int l, const DecView& v, int t0) {  // layer l's alignment heads
    for (int h = 0; h < 32; ++h) p.cap_sel[h] = -1;
    const int n_sel = (int)al.pairs.size() / 2;
    bool any = false;
    for (int k = 0; k < n_sel; ++k)
        if (al.pairs[2 * k] == l) {
            p.cap_sel[al.pairs[2 * k + 1]] = (signed char)k;
            any = true;
        }
    if (any && al.ragged) {  // an align pass's chunk: rows [t0, t0 + P) of the row map (single-lane: b0 = 0)
        p.cap = al.cap.as<float>();
        p.cap_map = al.map.as<int>() + (size_t)std::max(t0, 0) * v.nb;
        p.cap_nsel = n_sel;
    } else if (any) {
        p.cap_row_stride = (long)al.L * n_sel * 64;
        p.cap = al.cap.as<float>() + (size_t)v.b0 * p.cap_row_stride;
        p.cap_step0 = al.n_prompt;
        p.cap_steps = al.L;
        p.cap_nsel = n_sel;
        p.ctl = v.ctl;  // the step index comes from the cache length (the row map needs none)
    }
}
static void add_gelu_t(DecLinearParams& p, int gelu_mode) {  // GELU, stored in the operand dtype for the next MFMA
    p.act = 1;
    p.gelu_mode = gelu_mode;
    p.out_is_t = 1;
}
static void add_argmax_partials(DecLinearParams& p, wm_state* s, const DecView& v, const float* mask, const TsRules* rules) {
    p.amax_val = lane_ptr<float>(s->amax_val, v, s->npart);
    p.amax_idx = lane_ptr<int>(s->amax_idx, v, s->npart);
    p.amax_stride = s->npart;
    p.amax_mask = mask;
    if (rules && rules->tb > 0) {  // timestamp rules: split the candidates by the utterances' admissible ranges
        p.ts_state = lane_ptr<TsState>(s->ts_state, v, 1);
        p.ts_begin = rules->tb;
        p.ts_val = lane_ptr<float>(s->ts_val, v, s->npart);
        p.ts_idx = lane_ptr<int>(s->ts_idx, v, s->npart);
        p.ts_m = lane_ptr<float>(s->ts_m, v, s->npart);
        p.ts_s = lane_ptr<float>(s->ts_s, v, s->npart);
    }
    if (s->lp.on) p.lp_s = lane_ptr<float>(s->lp.part_s, v, s->npart);
    if (s->rp.on) {  // repetition processors: the rows' sets, ahead of the mask and the ranges
        p.rp_seen = lane_ptr<unsigned>(s->rp.seen, v, s->rp.words);
        p.rp_ban = lane_ptr<unsigned>(s->rp.ban, v, s->rp.words);
        p.rp_ctl = s->rp.ctl.as<RepeatCtl>();
        p.rp_words = s->rp.words;
        if (s->rp.sb) {
            p.sb_hit = lane_ptr<unsigned>(s->rp.hit, v, s->rp.words);
            p.sb_val = lane_ptr<SeqSlot>(s->rp.val, v, SEQ_BIAS_MAX);
            p.sb_ctl = s->rp.sbctl.as<SeqBiasCtl>();
        }
    }
}
// start of a pass with the repetition processors, behind the lane's init-tokens launch
static void repeat_init(wm_state* s, const DecView& v) {
    RepeatInitParams r{};
    r.seen = lane_ptr<unsigned>(s->rp.seen, v, s->rp.words);
    r.ban = lane_ptr<unsigned>(s->rp.ban, v, s->rp.words);
    r.words = s->rp.words;
    r.B = v.nb;
    r.ctl = s->rp.ctl.as<RepeatCtl>();
    r.penalty = s->rp.ask.penalty;
    r.ngram = s->rp.ask.ngram;
    r.out_tokens = lane_ptr<int>(s->out_tokens, v, s->out_stride);
    r.out_stride = s->out_stride;
    r.n_tokens = lane_ptr<int>(s->n_tokens, v, 1);
    launch_repeat_init(r, v.st);
}
// start of a pass with sequence bias / bad words, behind the lane's init-tokens launch; eot: the pass's, whose length-1 ban is dropped
static int seq_bias_init(wm_state* s, const DecView& v, int eot) {
    SeqBiasInitParams r{};
    r.hit = lane_ptr<unsigned>(s->rp.hit, v, s->rp.words);
    r.val = lane_ptr<SeqSlot>(s->rp.val, v, SEQ_BIAS_MAX);
    r.words = s->rp.words;
    r.B = v.nb;
    r.ctl = s->rp.sbctl.as<SeqBiasCtl>();
    r.table = s->rp.ask.sb->ctl(eot);
    r.out_tokens = lane_ptr<int>(s->out_tokens, v, s->out_stride);
    r.out_stride = s->out_stride;
    r.n_tokens = lane_ptr<int>(s->n_tokens, v, 1);
    LCHK(launch_seq_bias_init(r, v.st));
    return 0;
}
// start of a pass with a phrase-list constraint, behind repeat_init (and seq_bias_init); eot: the pass's, allowed where a phrase ends
static int constraint_init(wm_model* m, wm_state* s, const DecView& v, int eot) {
    ConstraintInitParams r{};
    r.ban = lane_ptr<unsigned>(s->rp.ban, v, s->rp.words);
    r.seen = lane_ptr<unsigned>(s->rp.seen, v, s->rp.words);
    r.words = s->rp.words;
    r.B = v.nb;
    r.vocab = m->cfg.dims.vocab;
    r.node = lane_ptr<int>(s->rp.node, v, 1);
    r.match = lane_ptr<int>(s->rp.match, v, 1);
    r.ctl = s->rp.ctctl.as<ConstraintCtl>();
    r.table = s->rp.ask.ct->ctl(eot);
    r.ngram = s->rp.ask.ngram;
    r.out_tokens = lane_ptr<int>(s->out_tokens, v, s->out_stride);
    r.out_stride = s->out_stride;
    r.n_tokens = lane_ptr<int>(s->n_tokens, v, 1);
    LCHK(launch_constraint_init(r, v.st));
    return 0;
}
// LN1 -> q | k,v appended to the cache   (layers.mojo:118-147)
DecLinearParams qkv_block(wm_model* m, wm_state* s, const DecView& v, int l, int P) {
    const wm_dims& c = m->cfg.dims;
    const DecLayer& w = m->dec[l];
    DecLinearParams p = linear_block(lane_ptr<float>(s->dx, v, c.d_model), w.ln1_g.as<float>(), w.ln1_b.as<float>(), w.sqkv_w.p, w.sqkv_b.as<float>(),
                                  3 * c.d_model, c.d_model, v.nb * P, lane_ptr<float>(s->dq, v, c.d_model), c.d_model);
    add_cache_append(p, m, s, v, l, P);
    return p;
}
// x += in·Wᵀ + b, `in` in operand dtype (what the attention / fc1 launches hand over)
DecLinearParams proj_residual_block(wm_model* m, wm_state* s, const DecView& v, int P, const float* in, int K, const DevBuf& W, const DevBuf& bias) {
    const wm_dims& c = m->cfg.dims;
    float* dx = lane_ptr<float>(s->dx, v, c.d_model);
    DecLinearParams p = linear_block(in, nullptr, nullptr, W.p, bias.as<float>(), c.d_model, K, v.nb * P, dx, c.d_model);
    p.x_is_t = 1;
    p.residual = dx;
    p.ldr = c.d_model;
    return p;
}

int decode_core(wm_model* m, wm_state* s, const DecView& v, const DecPass& a) {
    const wm_dims& c = m->cfg.dims;
    const int T = dec_dtype(m->cfg), KV = m->cfg.kv_dtype;  // T: the decoder's operand dtype
    const int P = a.P, B = v.nb * P;  // B: activation rows of this pass
    const int qB = P > 1 ? v.nb : 0;  // position-major row mapping on
    const size_t d = c.d_model;
    hipStream_t st = v.st;
    float* dx = lane_ptr<float>(s->dx, v, d);
    float* dq = lane_ptr<float>(s->dq, v, d);
    // attention output / MLP hidden rows: operand dtype T (fp32 buffers, used at T's width)
    float* dattn = (float*)off_bytes(s->dattn, (size_t)v.b0 * d * dt_size(T));
    float* dhid = (float*)off_bytes(s->dhid, (size_t)v.b0 * c.ffn * dt_size(T));
    if (a.embed) {
        const size_t row0 = a.t0 >= 0 ? (size_t)a.t0 * v.nb : 0;  // the pass's first row of tok_rows / pos_rows
        const bool rows = a.t0 >= 0 || P > 1;
        launch_dec_embed(m->tok_emb_f.as<float>(), m->dec_pos.as<float>(), rows ? s->tok_rows.as<int>() + row0 : lane_ptr<int>(s->tok, v, 1),
                         rows ? s->pos_rows.as<int>() + row0 : lane_ptr<int>(s->pos, v, 1), dx, B, c.d_model, st);
    }
    for (int l = 0; l < c.n_layers; ++l) {
        DecLayer& w = m->dec[l];
        WMCHK(dec_linear_dispatch(T, qkv_block(m, s, v, l, P), st));
        {  // self-attention over current_len+1 cached rows   (layers.mojo:186-272)
            AttnDecParams q{};
            q.q = dq;
            q.K = self_kv_rows(m, s, v, l, 0);
            q.V = self_kv_rows(m, s, v, l, 1);
            q.batch_stride = (long)((size_t)c.n_text_ctx * d);
            q.n_keys = -1;
            q.q_B = qB;
            q.ctl = v.ctl;
            q.nsplit = 1;
            q.scale = ATTN_SCALE;
            q.direct_out = dattn;
            q.out_dtype = T;
            q.H = c.n_heads;
            q.d = c.d_model;
            q.B = B;
            // per-row prompts: every utterance sweeps its own key window [key_lo, len + 1 (+ t))
            WMCHK(attn_decode_dispatch(KV, q, st, s->rw.on && a.key_window ? lane_ptr<int>(s->rw.key_lo, v, 1) : nullptr));
        }
        WMCHK(dec_linear_dispatch(T, proj_residual_block(m, s, v, P, dattn, c.d_model, w.so_w, w.so_b), st));
        {  // LNx -> cross q
            DecLinearParams p = linear_block(dx, w.lnx_g.as<float>(), w.lnx_b.as<float>(), w.cq_w.p, w.cq_b.as<float>(), c.d_model, c.d_model, B, dq, c.d_model);
            if (a.capture && s->al.on) add_align_capture(p, s->al, l, v, a.t0);
            WMCHK(dec_linear_dispatch(T, p, st));
        }
        WMCHK(launch_cross_attn(m, s, l, v, P));
        // (merging the chunk partials inside the projection's prologue was measured 14 us per layer SLOWER than this
        // 3 us launch: 96 workgroups each re-reading 295 KB of partials)
        if (m->xattn)
            WMCHK(cross_attn_merge(m, s, l, v, P, dattn, T));
        else
            launch_attn_combine(lane_ptr<float>(s->part_o, v, s->nsplit * d), lane_ptr<float>(s->part_ml, v, (size_t)s->nsplit * c.n_heads * 2), dattn, T, B,
                                s->nsplit, c.n_heads, c.d_model, st, (long long*)m->ts_buf.p, s->trace_id);
        WMCHK(dec_linear_dispatch(T, proj_residual_block(m, s, v, P, dattn, c.d_model, w.co_w, w.co_b), st));
        {  // LN2 -> fc1 + GELU
            DecLinearParams p = linear_block(dx, w.ln2_g.as<float>(), w.ln2_b.as<float>(), w.fc1_w.p, w.fc1_b.as<float>(), c.ffn, c.d_model, B, dhid, c.ffn);
            add_gelu_t(p, m->cfg.gelu_mode);
            WMCHK(dec_linear_dispatch(T, p, st));
        }
        WMCHK(dec_linear_dispatch(T, proj_residual_block(m, s, v, P, dhid, c.ffn, w.fc2_w, w.fc2_b), st));
    }
    if (a.logits != Logits::none) {  // final LN + tied-embedding logits (whisper.mojo:156-166), no bias, rows of the last position
        const VocabHead h = vocab_head(m);
        DecLinearParams p = linear_block(dx + (size_t)(P - 1) * v.nb * d, h.ln_g, h.ln_b, h.emb, nullptr, h.vocab, h.d_model, v.nb,
                                      a.logits == Logits::full || s->tk.k > 0 ? lane_ptr<float>(s->logits, v, m->Vpad) : nullptr, m->Vpad);
        add_argmax_partials(p, s, v, a.mask, a.rules);  // (top-k alternatives: the selection launch reads the stored, processed rows)
        p.ts = (long long*)m->ts_buf.p;
        p.ts_id = s->trace_id;
        int lrc = 0;
        DISPATCH_DT(T, TT, lrc = launch_dec_logits<TT>(p, st));
        LCHK(lrc);
    }
    return 0;
}

// The fused argmax's second stage, in its three uses.  wm_decode_step: the next id of every row, nothing recorded, no stop rule
static ArgmaxParams argmax_peek(wm_model* m, wm_state* s, const DecView& v) {
    ArgmaxParams a{};
    a.logits = lane_ptr<float>(s->logits, v, m->Vpad);
    a.pval = lane_ptr<float>(s->amax_val, v, s->npart);
    a.pidx = lane_ptr<int>(s->amax_idx, v, s->npart);
    a.npart = s->npart;
    a.ldl = m->Vpad;
    a.V = m->cfg.dims.vocab;
    a.B = v.nb;
    a.next = lane_ptr<int>(s->tok, v, 1);
    a.out_stride = s->out_stride;
    a.n_tokens = lane_ptr<int>(s->n_tokens, v, 1);
    a.finished = lane_ptr<int>(s->finished, v, 1);
    a.ctl = v.ctl;
    a.pos = lane_ptr<int>(s->pos, v, 1);
    a.ts = (long long*)m->ts_buf.p;
    a.ts_id = s->trace_id;
    a.eot = -1;
    a.ignore_eot = 1;
    return a;
}
// the end of a prefill: the first id goes into the pass's outputs (ids, log-probs, timestamp history); the cache length stays
static ArgmaxParams argmax_first_id(wm_model* m, wm_state* s, const DecView& v, int eot, int ignore_eot, const TsRules* rules) {
    ArgmaxParams a = argmax_peek(m, s, v);
    if (rules && rules->tb > 0) {
        a.ts_state = lane_ptr<TsState>(s->ts_state, v, 1);
        a.rules = *rules;
        a.ts_val = lane_ptr<float>(s->ts_val, v, s->npart);
        a.ts_idx = lane_ptr<int>(s->ts_idx, v, s->npart);
        a.ts_m = lane_ptr<float>(s->ts_m, v, s->npart);
        a.ts_s = lane_ptr<float>(s->ts_s, v, s->npart);
        a.ts_part0 = rules->tb / dec_logits_ids_per_part(m->cfg.dims.vocab);
    }
    a.out_tokens = lane_ptr<int>(s->out_tokens, v, s->out_stride);
    if (s->lp.on) {
        a.lp_s = lane_ptr<float>(s->lp.part_s, v, s->npart);
        a.logprobs = lane_ptr<float>(s->lp.table, v, s->out_stride);
        a.lp_sum = lane_ptr<float>(s->lp.sum, v, 1);
        if (s->tk.k > 0) a.tk_rows = lane_ptr<TopkRow>(s->tk.rows, v, 1);
    }
    if (s->rp.on) {
        a.rp_seen = lane_ptr<unsigned>(s->rp.seen, v, s->rp.words);
        a.rp_ban = lane_ptr<unsigned>(s->rp.ban, v, s->rp.words);
        a.rp_ctl = s->rp.ctl.as<RepeatCtl>();
        a.rp_words = s->rp.words;
        if (s->rp.sb) {
            a.sb_hit = lane_ptr<unsigned>(s->rp.hit, v, s->rp.words);
            a.sb_val = lane_ptr<SeqSlot>(s->rp.val, v, SEQ_BIAS_MAX);
            a.sb_ctl = s->rp.sbctl.as<SeqBiasCtl>();
        }
    }
    a.eot = eot;
    a.ignore_eot = ignore_eot;
    return a;
}
// The argmax launch that records an id (a = argmax_first_id / argmax_loop_step): under a phrase-list constraint the instantiation
// that also moves the rows' trie nodes, else the launch as it always was.
static int launch_argmax_id(wm_state* s, const DecView& v, const ArgmaxParams& a) {
    if (!s->rp.ct) return launch_argmax_step(a, v.st);
    ArgmaxCtParams c{};
    static_cast<ArgmaxParams&>(c) = a;
    c.ct_node = lane_ptr<int>(s->rp.node, v, 1);
    c.ct_match = lane_ptr<int>(s->rp.match, v, 1);
    c.ct_ctl = s->rp.ctctl.as<ConstraintCtl>();
    return launch_argmax_step_ct(c, v.st);
}
// Top-k alternatives: the selection launch behind an argmax launch that recorded an id — the k best of each row's stored
// logits under `mask` and the ranges the argmax left in the row's TopkRow, into the tables' entry beside the id.  k = 0: nothing.
static int topk_select(wm_model* m, wm_state* s, const DecView& v, const float* mask) {
    if (s->tk.k <= 0) return 0;
    TopkSelectParams q{};
    q.logits = lane_ptr<float>(s->logits, v, m->Vpad);
    q.ldl = m->Vpad;
    q.V = m->cfg.dims.vocab;
    q.B = v.nb;
    q.mask = mask;
    q.rows = lane_ptr<TopkRow>(s->tk.rows, v, 1);
    q.k = s->tk.k;
    q.ids = lane_ptr<int>(s->tk.ids, v, (size_t)s->out_stride * s->tk.k);
    q.lps = lane_ptr<float>(s->tk.lps, v, (size_t)s->out_stride * s->tk.k);
    LCHK(launch_topk_select(q, v.st));
    return 0;
}
// a step of the greedy loop: also advances the cache length, reports progress to the host and writes the next step's input row
static ArgmaxParams argmax_loop_step(wm_model* m, wm_state* s, const DecView& v, int eot, int ignore_eot, const TsRules* rules) {
    ArgmaxParams a = argmax_first_id(m, s, v, eot, ignore_eot, rules);
    a.advance = 1;
    a.host_progress = s->d_prog;
    a.emb_tok = m->tok_emb_f.as<float>();
    a.emb_pos = m->dec_pos.as<float>();
    a.emb_out = lane_ptr<float>(s->dx, v, m->cfg.dims.d_model);
    a.d = m->cfg.dims.d_model;
    a.max_pos = m->cfg.dims.n_text_ctx - 1;
    return a;
}

extern "C" int wm_decode_step(wm_model* m, wm_state* s, const int32_t* tokens, int q_len, const int32_t* start_pos,
                              float* logits, int32_t* next) {
    if (!m || !s || !tokens || !start_pos || q_len <= 0) return fail(WM_E_ARG, "bad argument");
    WMCHK(check_state(m, s, -1));
    if (!s->has_enc) return fail(WM_E_STATE, "no encoder output in this state (call wm_encode first)");
    const wm_dims& c = m->cfg.dims;
    const int B = s->B;
    if (s->host_len + q_len > c.n_text_ctx) return fail(WM_E_STATE, "KV cache full (%d + %d > %d)", s->host_len, q_len, c.n_text_ctx);
    for (int b = 0; b < B; ++b) {
        if (start_pos[b] < 0 || start_pos[b] + q_len > c.n_text_ctx) return fail(WM_E_ARG, "start_pos[%d]=%d out of range", b, start_pos[b]);
        for (int i = 0; i < q_len; ++i)
            if (tokens[b * q_len + i] < 0 || tokens[b * q_len + i] >= c.vocab) return fail(WM_E_ARG, "token id out of range");
    }
    HIPCHK(hipSetDevice(m->device));
    hipStream_t st = m->stream;
    const DecView v = whole_batch(m, s);
    std::vector<int32_t> col(B), pos(B);
    DecPass pass;
    pass.logits = Logits::full;  // for the caller, of the last position
    if (q_len > 1 && q_len <= wm_state::PREFILL_MAX) {  // the q_len block of whisper.mojo:195 as ONE position-major pass
        std::vector<int32_t> trow((size_t)q_len * B), prow((size_t)q_len * B);
        for (int i = 0; i < q_len; ++i)
            for (int b = 0; b < B; ++b) {
                trow[(size_t)i * B + b] = tokens[b * q_len + i];
                prow[(size_t)i * B + b] = start_pos[b] + i;
            }
        HIPCHK(hipMemcpyAsync(s->tok_rows.p, trow.data(), trow.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(s->pos_rows.p, prow.data(), prow.size() * 4, hipMemcpyHostToDevice, st));
        launch_set_step(v.ctl, s->host_len, 1, nullptr, 0, nullptr, 0, B, st);
        pass.P = q_len;
        WMCHK(decode_core(m, s, v, pass));
        HIPCHK(hipGetLastError());         // a launch that failed (bad configuration, LDS attribute) is reported here
        HIPCHK(hipStreamSynchronize(st));  // trow / prow go out of scope
        s->host_len += q_len;
        q_len = 0;
    }
    for (int i = 0; i < q_len; ++i) {
        for (int b = 0; b < B; ++b) {
            col[b] = tokens[b * q_len + i];
            pos[b] = start_pos[b] + i;
        }
        HIPCHK(hipMemcpyAsync(s->tok.p, col.data(), B * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(s->pos.p, pos.data(), B * 4, hipMemcpyHostToDevice, st));
        launch_set_step(v.ctl, s->host_len, 1, nullptr, 0, nullptr, 0, B, st);
        pass.logits = i == q_len - 1 ? Logits::full : Logits::none;
        WMCHK(decode_core(m, s, v, pass));
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));  // col/pos are reused next iteration
        s->host_len += 1;
    }
    launch_set_step(v.ctl, s->host_len, 1, nullptr, 0, nullptr, 0, B, st);
    if (next) {
        launch_argmax_step(argmax_peek(m, s, v), st);
        HIPCHK(hipMemcpyAsync(next, s->tok.p, B * 4, hipMemcpyDeviceToHost, st));
    }
    if (logits)
        HIPCHK(hipMemcpy2DAsync(logits, (size_t)c.vocab * 4, s->logits.p, (size_t)m->Vpad * 4, (size_t)c.vocab * 4, B, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- greedy-loop enqueue machinery (used by transcribe_decode and the loop pump) -----------------------------------------------
static const int LOOP_CHUNK = 8;  // graph replays per sub-chunk; two sub-chunks (16 steps) are queued ahead of the GPU

// One step of the greedy loop for view v as s->step describes it: the decoder pass and its argmax.  The only place that pairs
// them — transcribe_decode captures this into the lanes' graphs, enqueue_loop_steps launches it where there is no graph.
static int loop_step(wm_model* m, wm_state* s, const DecView& v) {
    const wm_state::StepKey& k = s->step;
    DecPass step;
    step.embed = false;
    step.logits = Logits::partials;
    step.mask = s->mask_steady.as<float>();
    step.rules = &k.rules;  // (tb <= 0: off, as every reader of the rules checks)
    step.capture = true;
    WMCHK(decode_core(m, s, v, step));
    LCHK(launch_argmax_id(s, v, argmax_loop_step(m, s, v, k.eot, k.ignore_eot, &k.rules)));
    if (k.top_k > 0) WMCHK(topk_select(m, s, v, step.mask));
    return 0;
}

// n more steps of the pending pass's loop on the state's lane streams (captured graph, or eager launches in the developer build)
static int enqueue_loop_steps(wm_model* m, wm_state* s, int n) {
    for (int k = 0; k < n; ++k, ++s->loop_enq) {
        const int it = s->loop_enq;
        for (auto& ln : s->lanes) {
            if (trace_events_on() && it % 10 == 9) trace_mark(ln.st, "state %p lane %d step %d", (void*)s, ln.b0, it);
            if (ln.graph[0] && s->graphs_valid) {
                const hipError_t e = hipGraphLaunch(ln.graph[it % wm_state::Lane::NEXEC], ln.st);
                if (e != hipSuccess) return fail(WM_E_HIP, "hipGraphLaunch: %s", hipGetErrorString(e));
            } else {
                WMCHK(loop_step(m, s, DecView{ln.b0, ln.nb, ln.st, ln.ctl}));
            }
        }
    }
    return 0;
}
// the pending pass is fully enqueued: its completion events go behind the last step
static int finish_enqueue(wm_model* m, wm_state* s) {
    int rc = 0;
    if (s->al.on) {  // token timestamps: the post-loop kernels go behind the last step, before the pass's completion events
        for (size_t i = 1; i < s->lanes.size() && !rc; ++i) {
            hipError_t e = hipEventRecord(s->lanes[i].done, s->lanes[i].st);
            if (e == hipSuccess) e = hipStreamWaitEvent(s->lanes[0].st, s->lanes[i].done, 0);
            if (e != hipSuccess) rc = fail(WM_E_HIP, "align wait: %s", hipGetErrorString(e));
        }
        if (!rc) rc = enqueue_align(m, s);
    }
    for (auto& ln : s->lanes) {
        trace_mark(ln.st, "state %p lane %d decode end", (void*)s, ln.b0);
        const hipError_t e = hipEventRecord(ln.done, ln.st);
        if (e != hipSuccess && !rc) rc = fail(WM_E_HIP, "hipEventRecord: %s", hipGetErrorString(e));
    }
    if (!rc && hipGetLastError() != hipSuccess) rc = fail(WM_E_HIP, "a launch of the greedy loop failed");
    s->last_steps = s->loop_enq;
    if (rc && !s->enq_rc) {
        s->enq_rc = rc;
        s->enq_err = g_err;
    }
    s->enq_done.store(true);
    return rc;
}
static int enqueue_chunk(wm_model* m, wm_state* s) {
    const int n = std::min(LOOP_CHUNK, s->loop_total - s->loop_enq);
    WMCHK(enqueue_loop_steps(m, s, n));
    HIPCHK(hipEventRecord(s->chunk_ev[s->chunk_k & 1], s->lanes[0].st));
    ++s->chunk_k;
    return 0;
}
// One decision of the loop pump for state s: once sub-chunk k-2 has completed, either stop (every utterance finished, or the loop
// bound reached) or enqueue sub-chunk k.  Returns 1 when it did something, 0 when sub-chunk k-2 is still running (non-blocking
// form), < 0 on error (the pass is then closed with enq_rc set).
static int pump_step(wm_model* m, wm_state* s, bool block) {
    hipEvent_t ev = s->chunk_ev[s->chunk_k & 1];  // recorded behind sub-chunk chunk_k - 2
    hipError_t e = block ? hipEventSynchronize(ev) : hipEventQuery(ev);
    if (e == hipErrorNotReady) return 0;
    int rc = e == hipSuccess ? 0 : fail(WM_E_HIP, "loop pump: %s", hipGetErrorString(e));
    if (!rc) {
        const bool all_done = s->h_prog[0] >= s->B;  // a lower bound of the finished count: never stops a running utterance
        if (all_done || s->loop_enq >= s->loop_total) {
            rc = finish_enqueue(m, s);
            return rc ? -1 : 1;
        }
        rc = enqueue_chunk(m, s);
        if (!rc) return 1;
    }
    s->enq_rc = rc;
    s->enq_err = g_err;
    (void)finish_enqueue(m, s);
    return -1;
}
static void pump_main(wm_model* m) {
    (void)hipSetDevice(m->device);
    std::unique_lock<std::mutex> lk(m->pump_mu);
    for (;;) {
        m->pump_cv.wait(lk, [&] { return m->pump_quit || !m->pump_work.empty(); });
        if (m->pump_quit) return;
        bool progressed = false;
        for (size_t i = 0; i < m->pump_work.size();) {
            wm_state* s = m->pump_work[i];
            if (pump_step(m, s, false) != 0) progressed = true;
            if (s->enq_done.load()) {
                m->pump_work.erase(m->pump_work.begin() + (long)i);
                m->pump_cv.notify_all();  // wm_transcribe_wait may be waiting for this pass to be fully enqueued
            } else {
                ++i;
            }
        }
        if (!progressed) {  // every pending sub-chunk still running: they take milliseconds
            lk.unlock();
            std::this_thread::sleep_for(std::chrono::microseconds(100));
            lk.lock();
        }
    }
}

// No-speech probe.  capture: after the prefill pass that holds the <|startoftranscript|> position, keep that position's
// residual rows (row_off: its first row in the pass's position-major activations).  probe: after the prefill, one vocabulary sweep
// over the kept rows — the log-prob instantiation of the logits kernel a decode step of this state picks, no mask, no ranges, its
// partials in the probe's own buffers — and the finish kernel.  Both go on the lane's stream, outside the captured step graph.
static void ns_capture(wm_model* m, wm_state* s, const DecView& v, size_t row_off) {
    const size_t d = m->cfg.dims.d_model;
    launch_no_speech_capture(lane_ptr<float>(s->dx, v, d) + row_off * d, lane_ptr<float>(s->ns.x, v, d), v.nb, (int)d, v.st);
}
int ns_sweep(int T, const float* x, const VocabHead& h, int B, int npart, float* pmax, int* pidx, float* psum, int token, float* prob,
             float* lse, hipStream_t st) {
    DecLinearParams p = linear_block(x, h.ln_g, h.ln_b, h.emb, nullptr, h.vocab, h.d_model, B, nullptr, (h.vocab + 3) / 4 * 4);
    p.amax_val = pmax;
    p.amax_idx = pidx;
    p.amax_stride = npart;
    p.lp_s = psum;
    int lrc = 0;
    DISPATCH_DT(T, TT, lrc = launch_dec_logits<TT>(p, st));
    LCHK(lrc);
    NoSpeechParams q{};
    q.x = x;
    q.ldx = h.d_model;
    q.ln_g = h.ln_g;
    q.ln_b = h.ln_b;
    q.emb = h.emb;
    q.K = h.d_model;
    q.token = token;
    q.B = B;
    q.pmax = pmax;
    q.psum = psum;
    q.npart = npart;
    q.stride = npart;
    q.prob = prob;
    q.lse = lse;
    DISPATCH_DT(T, TT, launch_no_speech_finish<TT>(q, st));
    return 0;
}
static int ns_probe(wm_model* m, wm_state* s, const DecView& v) {
    const wm_state::Ns& ns = s->ns;
    return ns_sweep(dec_dtype(m->cfg), lane_ptr<float>(ns.x, v, m->cfg.dims.d_model), vocab_head(m), v.nb, s->npart, lane_ptr<float>(ns.pmax, v, s->npart),
                    lane_ptr<int>(ns.pidx, v, s->npart), lane_ptr<float>(ns.psum, v, s->npart), ns.token, lane_ptr<float>(ns.prob, v, 1),
                    lane_ptr<float>(ns.lse, v, 1), v.st);
}

// Language detection, after the encoder on a single-lane state: one decoder pass over [sot] at position 0 for all rows
// (cache length 0, every row attends only to itself, no key window, no logits; its K/V rows in cache slot 0 are overwritten by the
// prefill that follows), its residual rows kept in lg.x, then lang_detect_kernel.  patch: the device prompt table whose language
// slots (lg.col) receive the ids, or null.  All on the lane's stream; nothing is read back.
static int lang_pass(wm_model* m, wm_state* s, const DecView& v, int* patch, int patch_stride) {
    const wm_dims& c = m->cfg.dims;
    const int T = dec_dtype(m->cfg);
    wm_state::Lang& lg = s->lg;
    HIPCHK(hipMemcpyAsync(lg.ids.p, lg.h_ids.data(), (size_t)lg.n * 4, hipMemcpyHostToDevice, v.st));
    if (patch) HIPCHK(hipMemcpyAsync(lane_ptr<int>(lg.col, v, 1), lg.h_col.data() + v.b0, (size_t)v.nb * 4, hipMemcpyHostToDevice, v.st));
    launch_set_step(v.ctl, 0, 1, lane_ptr<int>(s->pos, v, 1), 0, lane_ptr<int>(s->tok, v, 1), lg.sot, v.nb, v.st);
    DecPass sot;
    sot.key_window = false;
    WMCHK(decode_core(m, s, v, sot));
    launch_no_speech_capture(lane_ptr<float>(s->dx, v, c.d_model), lane_ptr<float>(lg.x, v, c.d_model), v.nb, c.d_model, v.st);
    const VocabHead h = vocab_head(m);
    LangDetectParams q{};
    q.x = lane_ptr<float>(lg.x, v, c.d_model);
    q.ldx = c.d_model;
    q.ln_g = h.ln_g;
    q.ln_b = h.ln_b;
    q.emb = h.emb;
    q.lang_ids = lg.ids.as<int>();
    q.n_lang = lg.n;
    q.K = h.d_model;
    q.B = v.nb;
    q.lang_out = lane_ptr<int>(lg.out, v, 1);
    q.probs = lane_ptr<float>(lg.probs, v, lg.n);
    q.patch = patch ? patch + (size_t)v.b0 * patch_stride : nullptr;
    q.patch_stride = patch_stride;
    q.patch_col = lane_ptr<int>(lg.col, v, 1);
    DISPATCH_DT(T, TT, launch_lang_detect<TT>(q, v.st));
    return 0;
}

// Per-row prompts, the start of a pass on a single-lane state: prompt table and lengths to the device, tokens /
// key windows / prefill rows from them, the prefill in chunks of PREFILL_MAX positions through the position-major pass (the rows
// end together at position Lmax; logits for the last chunk only: every row's last position is real), the first id, and the per-row
// positions of the first loop step.  ip: the pass's InitTokensParams without the prompt.
static int prefill_rows(wm_model* m, wm_state* s, const DecView& v, InitTokensParams ip, const wm_decode_opts* o, const TsRules* rp) {
    wm_state::Rows& rw = s->rw;
    const int Lmax = rw.Lmax;
    HIPCHK(hipMemcpyAsync(rw.table.p, rw.h_table.data(), rw.h_table.size() * 4, hipMemcpyHostToDevice, v.st));
    HIPCHK(hipMemcpyAsync(rw.len.p, rw.h_len.data(), rw.h_len.size() * 4, hipMemcpyHostToDevice, v.st));
    if (s->lg.on) WMCHK(lang_pass(m, s, v, rw.table.as<int>(), rw.stride));  // the table's language slots come from the device (§19)
    ip.tok_rows = s->tok_rows.as<int>();
    ip.pos_rows = s->pos_rows.as<int>();
    launch_init_tokens_rows(ip, RowPromptParams{rw.table.as<int>(), rw.len.as<int>(), rw.stride, Lmax, rw.key_lo.as<int>()}, v.st);
    if (s->rp.on) repeat_init(s, v);  // each row's own prompt, a detected language included
    if (s->rp.sb) WMCHK(seq_bias_init(s, v, o->eot));
    if (s->rp.ct) WMCHK(constraint_init(m, s, v, o->eot));
    for (int t0 = 0; t0 < Lmax; t0 += wm_state::PREFILL_MAX) {
        const int P = std::min<int>(wm_state::PREFILL_MAX, Lmax - t0);
        if (t0) launch_set_step(v.ctl, t0, 1, nullptr, 0, nullptr, 0, v.nb, v.st);
        DecPass chunk;
        chunk.P = P;
        chunk.t0 = t0;
        chunk.logits = t0 + P == Lmax ? Logits::partials : Logits::none;
        chunk.mask = s->mask_begin.as<float>();
        chunk.rules = rp;
        WMCHK(decode_core(m, s, v, chunk));
        // the rows end together, so every row's <|startoftranscript|> sits in cache slot Lmax - n_init, whatever its own length
        const int t_sot = Lmax - s->ns.n_init;
        if (s->ns.on && t_sot >= t0 && t_sot < t0 + P) ns_capture(m, s, v, (size_t)(t_sot - t0) * v.nb);
    }
    LCHK(launch_argmax_id(s, v, argmax_first_id(m, s, v, o->eot, o->ignore_eot, rp)));
    WMCHK(topk_select(m, s, v, s->mask_begin.as<float>()));
    trace_mark(v.st, "state %p lane %d prefill end", (void*)s, v.b0);
    launch_set_rows_step(v.ctl, Lmax, lane_ptr<int>(s->pos, v, 1), rw.len.as<int>(), o->pos_mode == WM_POS_REF ? -1 : 0, v.nb, v.st);
    return 0;
}

// ---- Whisper.transcribe: whisper.mojo:184-223 ------------------------------------------------------------------------
// Enqueues the prompt prefill and the greedy loop for state s on its decode lane streams; returns without waiting.  The lanes
// first wait for the encoder (recorded on the stream it ran on).  Both entry points stop once every utterance has emitted eot
// (whisper.mojo:206-207): allow_poll = the synchronous one feeds its loop itself, sub-chunk by sub-chunk; the pipelined one
// hands the rest of the loop to the model's pump thread (see the enqueue machinery above).
static int transcribe_decode(wm_model* m, wm_state* s, const wm_decode_opts* o, bool allow_poll) {
    HIPCHK(hipEventRecord(s->enc_done, s->enc_stream ? s->enc_stream : m->stream));  // encoder + cross K/V of this state
    static const bool trace_phase = wm_env("WM_TRACE_HOST") != nullptr;
    const auto tp0 = std::chrono::steady_clock::now();
    static const bool no_graph = wm_env("WM_NO_GRAPH") != nullptr;
    s->step = wm_state::StepKey{};      // the loop step of this pass
    TsRules& rules = s->step.rules;  // timestamp rules of this pass (tb <= 0: off)
    rules.tb = o->timestamp_begin > 0 ? o->timestamp_begin : 0;
    rules.eos = o->eot;
    rules.max_init = o->max_initial_timestamp_index;
    rules.vocab = m->cfg.dims.vocab;
    const TsRules* rp = rules.tb > 0 ? &rules : nullptr;
    const int no_ts = rp ? o->no_timestamps_token : -1;
    s->shares_chip = !allow_poll;  // the pipelined entry (wm_transcribe_submit): other passes are, or will be, in flight
    s->step.eot = o->eot;
    s->step.ignore_eot = o->ignore_eot;
    s->step.shares_chip = s->shares_chip;
    if (s->al.on) s->step.cap = wm_state::StepKey::Cap{s->al.cap.p, s->al.L, s->al.n_prompt, s->al.pairs};
    s->step.rows = s->rw.on;
    s->step.lp = s->lp.on;
    s->step.rp = s->rp.on;
    s->step.sb = s->rp.sb;
    s->step.ct = s->rp.ct;
    s->step.top_k = s->tk.k;
    const bool recapture = !s->graphs_valid || !(s->graph_step == s->step);
    const int first_pos = o->pos_mode == WM_POS_REF ? o->n_prompt - 1 : o->n_prompt;
    // logit masks (§8f rank 4): rebuilt only when the id lists change; always passed (all-zero = the reference's raw argmax)
    {
        std::vector<int32_t> sup(o->suppress_tokens, o->suppress_tokens + (o->suppress_tokens ? o->n_suppress : 0));
        std::vector<int32_t> bsup(o->begin_suppress_tokens, o->begin_suppress_tokens + (o->begin_suppress_tokens ? o->n_begin_suppress : 0));
        if (!s->masks_valid || sup != s->sup_cached || bsup != s->bsup_cached || no_ts != s->no_ts_cached) {
            std::vector<float> ms(m->Vpad, 0.f), mb(m->Vpad, 0.f);
            if (no_ts >= 0 && no_ts < m->cfg.dims.vocab) ms[no_ts] = mb[no_ts] = -INFINITY;  // <|notimestamps|> is never emitted under the timestamp rules
            s->no_ts_cached = no_ts;
            for (int32_t id : sup)
                if (id >= 0 && id < m->cfg.dims.vocab) ms[id] = mb[id] = -INFINITY;
            for (int32_t id : bsup)
                if (id >= 0 && id < m->cfg.dims.vocab) mb[id] = -INFINITY;
            HIPCHK(hipMemcpy(s->mask_steady.p, ms.data(), ms.size() * 4, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(s->mask_begin.p, mb.data(), mb.size() * 4, hipMemcpyHostToDevice));
            s->sup_cached = sup;
            s->bsup_cached = bsup;
            s->masks_valid = true;
        }
    }
    InitTokensParams ip{};
    ip.n_prompt = o->n_prompt;
    if (!s->rw.on)  // (per-row prompts: o->n_prompt is the longest row's length, the ids come from the device table)
        for (int i = 0; i < o->n_prompt; ++i) ip.prompt[i] = o->prompt[i];
    for (auto& ln : s->lanes) {
        const DecView v{ln.b0, ln.nb, ln.st, ln.ctl};
        HIPCHK(hipStreamWaitEvent(v.st, s->enc_done, 0));
        trace_mark(v.st, "state %p lane %d decode start", (void*)s, v.b0);
        // tokens = prompt (whisper.mojo:187-191, 200-202); finished = 0; control block = 0
        ip.out_tokens = lane_ptr<int>(s->out_tokens, v, s->out_stride);
        ip.out_stride = s->out_stride;
        ip.n_tokens = lane_ptr<int>(s->n_tokens, v, 1);
        ip.finished = lane_ptr<int>(s->finished, v, 1);
        ip.ctl = v.ctl;
        ip.B = v.nb;
        ip.tok_rows = s->lanes.size() == 1 ? s->tok_rows.as<int>() : nullptr;
        ip.pos_rows = s->pos_rows.as<int>();
        ip.ts_state = rp ? lane_ptr<TsState>(s->ts_state, v, 1) : nullptr;
        ip.rules = rules;
        ip.logprobs = s->lp.on ? lane_ptr<float>(s->lp.table, v, s->out_stride) : nullptr;
        ip.lp_sum = s->lp.on ? lane_ptr<float>(s->lp.sum, v, 1) : nullptr;
        if (s->rw.on) {
            WMCHK(prefill_rows(m, s, v, ip, o, rp));
        } else {
            launch_init_tokens(ip, v.st);
            if (s->rp.on) repeat_init(s, v);
            if (s->rp.sb) WMCHK(seq_bias_init(s, v, o->eot));
            if (s->rp.ct) WMCHK(constraint_init(m, s, v, o->eot));
            // prefill (whisper.mojo:195, start_pos=0): the q_len = n_prompt causal block equals n_prompt single-token steps
            static const bool seq_prefill = wm_env("WM_SEQ_PREFILL") != nullptr;  // A/B: one pass per prompt position
            DecPass prompt;  // the last prompt position's logits, under the begin mask
            prompt.logits = Logits::partials;
            prompt.mask = s->mask_begin.as<float>();
            prompt.rules = rp;
            if (!seq_prefill && s->lanes.size() == 1 && o->n_prompt > 1 && o->n_prompt <= wm_state::PREFILL_MAX) {
                prompt.P = o->n_prompt;  // init_tokens filled tok_rows / pos_rows
                WMCHK(decode_core(m, s, v, prompt));
                if (s->ns.on) ns_capture(m, s, v, (size_t)(o->n_prompt - s->ns.n_init) * v.nb);
            } else {
                for (int i = 0; i < o->n_prompt; ++i) {
                    launch_set_step(v.ctl, i, 1, lane_ptr<int>(s->pos, v, 1), i, lane_ptr<int>(s->tok, v, 1), o->prompt[i], v.nb, v.st);
                    prompt.logits = i == o->n_prompt - 1 ? Logits::partials : Logits::none;
                    WMCHK(decode_core(m, s, v, prompt));
                    if (s->ns.on && i == o->n_prompt - s->ns.n_init) ns_capture(m, s, v, 0);
                }
            }
            LCHK(launch_argmax_id(s, v, argmax_first_id(m, s, v, o->eot, o->ignore_eot, rp)));  // :198-203
            WMCHK(topk_select(m, s, v, prompt.mask));
            trace_mark(v.st, "state %p lane %d prefill end", (void*)s, v.b0);
            // incremental steps: start_pos = current_len - 1 (reference, :217) or current_len (HF)
            launch_set_step(v.ctl, o->n_prompt, 1, lane_ptr<int>(s->pos, v, 1), first_pos, nullptr, 0, v.nb, v.st);
        }
        // input row of the first loop step; every later step's row is written by the preceding step's argmax launch
        launch_dec_embed(m->tok_emb_f.as<float>(), m->dec_pos.as<float>(), lane_ptr<int>(s->tok, v, 1), lane_ptr<int>(s->pos, v, 1),
                         lane_ptr<float>(s->dx, v, m->cfg.dims.d_model), v.nb, m->cfg.dims.d_model, v.st);
        if (s->ns.on) WMCHK(ns_probe(m, s, v));  // between prefill and loop, outside the captured step
        // steady state: one captured graph per lane = [37 decode-step launches + argmax/bookkeeping]; every per-step
        // quantity (token, position, cache length) lives in HBM, so the same graph is replayed for every token
        if (!no_graph && (recapture || !ln.graph[0])) {
            for (auto& ge : ln.graph) {
                if (ge) (void)hipGraphExecDestroy(ge);
                ge = nullptr;
            }
            hipGraph_t g = nullptr;
            HIPCHK(hipStreamBeginCapture(v.st, hipStreamCaptureModeThreadLocal));
            const int crc = loop_step(m, s, v);
            const hipError_t cap = hipStreamEndCapture(v.st, &g);  // always closed, also when a launcher refused
            if (crc) {
                if (g) (void)hipGraphDestroy(g);
                return crc;
            }
            HIPCHK(cap);
            hipError_t ge = hipSuccess;
            for (int k = 0; k < wm_state::Lane::NEXEC && ge == hipSuccess; ++k) ge = hipGraphInstantiate(&ln.graph[k], g, nullptr, nullptr, 0);
            (void)hipGraphDestroy(g);
            if (ge != hipSuccess) return fail(WM_E_HIP, "hipGraphInstantiate: %s", hipGetErrorString(ge));
        }
    }
    s->graphs_valid = !no_graph;
    s->graph_step = s->step;
    if (trace_phase) {
        for (auto& ln : s->lanes) (void)hipStreamSynchronize(ln.st);
        fprintf(stderr, "[wm] encoder wait + prefill (+graph capture if any): %.3f ms\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - tp0).count() * 1e3);
    }
    // The loop itself.  Fixed-length passes (ignore_eot: the bench's "fixed" mode) and short loops are enqueued whole.  With the
    // reference's stop rule the loop goes out in sub-chunks of LOOP_CHUNK graph replays, two sub-chunks ahead of the GPU; before
    // each further sub-chunk the host reads the (finished, length) pair the argmax launches write to pinned memory — no stream
    // synchronisation, the GPU never runs dry — and stops enqueueing once every utterance has emitted eot: "if next_token == eot:
    // break" (whisper.mojo:206-207) for the whole batch, at most two sub-chunks late.
    s->loop_total = o->max_loop;
    s->loop_enq = 0;
    s->chunk_k = 0;
    s->enq_rc = 0;
    s->enq_err.clear();
    s->h_prog[0] = 0;
    s->h_prog[1] = 0;
    const bool natural = !o->ignore_eot && s->lanes.size() == 1 && o->max_loop > 2 * LOOP_CHUNK && !no_graph;
    s->enq_done.store(false);
    if (!natural) {
        WMCHK(enqueue_loop_steps(m, s, o->max_loop));
        return finish_enqueue(m, s);
    }
    WMCHK(enqueue_chunk(m, s));
    WMCHK(enqueue_chunk(m, s));
    if (allow_poll) {  // the synchronous entry pumps its own loop
        while (!s->enq_done.load()) WMCHK(pump_step(m, s, true) < 0 ? s->enq_rc : 0);
        return 0;
    }
    {  // pipelined entry: the model's pump thread carries on; wm_transcribe_wait waits for it
        std::lock_guard<std::mutex> lk(m->pump_mu);
        if (!m->pump.joinable()) m->pump = std::thread(pump_main, m);
        m->pump_work.push_back(s);
    }
    m->pump_cv.notify_all();
    return 0;
}

int check_opts(wm_model* m, const wm_decode_opts* o, int B) {
    if (!o || B <= 0) return fail(WM_E_ARG, "bad argument");
    if (!o->prompt || o->n_prompt <= 0 || o->n_prompt > 16 || o->max_loop < 0) return fail(WM_E_ARG, "bad decode options (1 <= n_prompt <= 16)");
    if (o->n_suppress < 0 || o->n_begin_suppress < 0 || (o->n_suppress > 0 && !o->suppress_tokens) || (o->n_begin_suppress > 0 && !o->begin_suppress_tokens))
        return fail(WM_E_ARG, "bad suppress-token lists");
    const wm_dims& c = m->cfg.dims;
    if (o->timestamp_begin > 0) {
        if (o->timestamp_begin >= c.vocab) return fail(WM_E_ARG, "timestamp_begin %d is not a vocabulary id", o->timestamp_begin);
        if (o->no_timestamps_token >= c.vocab) return fail(WM_E_ARG, "no_timestamps_token out of range");
        if (o->eot < 0 || o->eot > o->timestamp_begin) return fail(WM_E_ARG, "timestamp rules need 0 <= eot <= timestamp_begin (eot is the processor's eos id)");
    }
    const int total = o->n_prompt + 1 + o->max_loop;
    if (total > c.n_text_ctx + 1 || total > OUT_STRIDE_MAX)
        return fail(WM_E_ARG, "n_prompt + 1 + max_loop = %d exceeds the decoder context %d", total, c.n_text_ctx);
    for (int i = 0; i < o->n_prompt; ++i)
        if (o->prompt[i] < 0 || o->prompt[i] >= c.vocab) return fail(WM_E_ARG, "prompt id out of range");
    return 0;
}

static int rows_setup(wm_model* m, wm_state* s, const RowPrompts* rows) {
    wm_state::Rows& rw = s->rw;
    rw.on = rows != nullptr;
    if (!rw.on) return 0;
    if (s->lanes.size() != 1) {
        rw.on = false;
        return fail(WM_E_ARG, "per-row prompts need a single-lane decode state");
    }
    const size_t B = s->B, ctx = m->cfg.dims.n_text_ctx;
    WMCHK(grow(rw.table, B * ctx * 4));
    WMCHK(grow(rw.len, B * 4));
    WMCHK(grow(rw.key_lo, B * 4));
    WMCHK(grow(s->tok_rows, B * ctx * 4));  // the whole prompt's position-major rows [Lmax][B], consumed chunk by chunk
    WMCHK(grow(s->pos_rows, B * ctx * 4));
    rw.Lmax = rows->Lmax;
    rw.stride = rows->Lmax;
    rw.h_table.assign(B * (size_t)rw.stride, 0);
    rw.h_len.assign(rows->len, rows->len + B);
    for (size_t b = 0; b < B; ++b) std::copy(rows->ids + b * rows->stride, rows->ids + b * rows->stride + rows->len[b], rw.h_table.begin() + b * rw.stride);
    return 0;
}
// Enqueues one whole pass (encoder, prefill, greedy loop) for ask.B utterances on state *slot (created / re-created on demand).
// ask.mel2 != null: a coalesced pair — *slot is a 2·(B/2)-row pair state.
int submit_on(wm_model* m, wm_state** slot, const PassAsk& ask) {
    const wm_dims& c = m->cfg.dims;
    const int B = ask.B;
    const wm_decode_opts* o = ask.opts;
    const bool lp = ask.lp;
    const std::vector<int32_t>* cols = ask.cols;
    const RowPrompts* rows = ask.rows;
    const NsAsk& ns = ask.ns;
    const LangAsk& lang = ask.lang;
    const ScoreAsk* score = ask.score;
    const int n_enc = score && score->n_utt > 0 ? score->n_utt : B;  // clips the encoder runs over: an n-best pass has fewer than rows
    if (score && (ask.mel2 || cols || rows || lp || ns.token >= 0 || lang.ids || dec_lanes_for(B) != 1))  // (refused by the entry points first)
        return fail(WM_E_ARG, "a score pass runs alone on a single-lane decode state");
    if (lang.ids && (ask.mel2 || cols || dec_lanes_for(B) != 1 || (!lang.only && !rows)))  // (refused by the entry points first)
        return fail(WM_E_ARG, "language detection needs a single-lane decode state and a per-row-prompt pass without token timestamps");
    if (ns.token >= 0 && (!lp || ns.token >= c.vocab || ns.n_init < 1 || ns.n_init > o->n_prompt))  // (refused by the entry points first)
        return fail(WM_E_ARG, "the no-speech probe needs a log-prob pass, a vocabulary id and 1 <= n_init <= prompt length");
    if (lp && (cols || dec_lanes_for(B) != 1))  // (the entry points refuse both before anything is touched; kept for internal callers)
        return fail(WM_E_ARG, "log-probabilities need a single-lane decode state and a pass without token timestamps");
    if ((ask.win && (!cols || ask.mel2)) || (rows && cols && !ask.win))  // (no entry point asks for either)
        return fail(WM_E_ARG, "per-row prompts take token timestamps in a long-form window pass only, and a window pass runs alone");
    HIPCHK(hipSetDevice(m->device));
    const bool pair = ask.mel2 != nullptr;
    // a pass that was submitted and not yet waited for owns the slot's state: refuse BEFORE touching it (re-creating the
    // state for another batch size would destroy graphs, streams and arenas under its running kernels)
    if (*slot && (*slot)->pending) return fail(WM_E_STATE, "this slot still holds a pass that was not waited for");
    if (!*slot || (*slot)->B != B) {
        if (*slot) wm_state_free(*slot);
        *slot = nullptr;
        WMCHK(state_new(m, B, slot, pair));
    }
    wm_state* s = *slot;
    WMCHK(rows_setup(m, s, rows));
    s->ns.on = ns.token >= 0;
    s->ns.token = ns.token;
    s->ns.n_init = ns.n_init;
    s->lg.on = lang.ids != nullptr && !lang.only;
    if (lang.ids) {
        s->lg.n = lang.n;
        s->lg.n_init = lang.n_init;
        s->lg.sot = lang.sot;
        s->lg.h_ids.assign(lang.ids, lang.ids + lang.n);
        s->lg.h_col.resize(B);
        for (int b = 0; b < B; ++b) s->lg.h_col[b] = rows ? rows->len[b] - lang.n_init + 1 : 0;
    }
    s->sc.on = false;
    s->nb.on = false;  // the row-to-clip map of an n-best pass serves that pass alone
    s->sc.timed = s->sc.timed_al = false;
    s->rp.on = ask.rp.on() && !score && !lang.only;  // greedy passes only: score / align are teacher-forced, detection reads raw logits
    if (s->rp.on) {
        s->rp.ask = ask.rp;
        s->rp.words = repeat_words(c.vocab);
        WMCHK(grow(s->rp.seen, (size_t)B * s->rp.words * 4));
        WMCHK(grow(s->rp.ban, (size_t)B * s->rp.words * 4));
        WMCHK(grow(s->rp.ctl, sizeof(RepeatCtl)));
    }
    s->rp.sb = s->rp.on && ask.rp.sb;
    if (s->rp.sb) {
        WMCHK(grow(s->rp.hit, (size_t)B * s->rp.words * 4));
        WMCHK(grow(s->rp.val, (size_t)B * SEQ_BIAS_MAX * sizeof(SeqSlot)));
        WMCHK(grow(s->rp.sbctl, sizeof(SeqBiasCtl)));
    } else {
        s->rp.ask.sb.reset();  // (a pass without the table holds no reference to one)
    }
    s->rp.ct = s->rp.on && ask.rp.ct;
    s->rp.ct_gen += 1;
    if (s->rp.ct) {
        WMCHK(grow(s->rp.node, (size_t)B * 4));
        WMCHK(grow(s->rp.match, (size_t)B * 4));
        WMCHK(grow(s->rp.ctctl, sizeof(ConstraintCtl)));
    } else {
        s->rp.ask.ct.reset();
    }
    s->lp.on = lp;
    s->tk.k = lp && !score && !lang.only ? ask.top_k : 0;  // the alternatives of a greedy log-prob pass; every other pass ignores the setting
    s->tk.gen += 1;
    if (lp) {
        if (rows)
            s->lp.n_prompt.assign(rows->len, rows->len + B);
        else
            s->lp.n_prompt.assign(B, o->n_prompt);
    }
    s->trace_id = slot == &m->cached ? 1 : (slot >= m->slots && slot < m->slots + (wm_model::NSLOT - 1)) ? 2 + (int)(slot - m->slots)
                : (slot == &m->lf.st[0] || slot == &m->lf.st[1]) ? 20 + (int)(slot - m->lf.st) : 10 + (int)(slot - m->pairs);
    // The whole pass — encoder, prefill, greedy loop — goes on the slot's own stream: four slots are then four hardware
    // queues, which is what the chip runs concurrently (a fifth queue, e.g. a shared encoder stream, lands on a pipe that
    // already serves one of them and the two take turns: 22.3 vs 20.8 ms per pass at four passes in flight).
    // WM_ENC_ON_MODEL_STREAM=1 restores the shared encoder stream for A/B runs.
    static const bool enc_on_lane = wm_env("WM_ENC_ON_MODEL_STREAM") == nullptr;
    hipStream_t est = enc_on_lane ? s->lanes[0].st : m->stream;
    s->has_enc = s->has_cross = false;
    s->host_len = 0;
    if (est != m->stream) {  // whatever produced the mel on the model stream (the log-mel front end) comes first
        HIPCHK(hipEventRecord(s->enc_done, m->stream));
        HIPCHK(hipStreamWaitEvent(est, s->enc_done, 0));
    }
    const size_t mel_floats = (size_t)c.n_mels * 2 * c.n_audio_ctx;  // per utterance
    const int B1 = pair ? B / 2 : n_enc;
    const float* mel_dev = ask.mel;
    if (!ask.mel_on_device) {
        HIPCHK(hipMemcpyAsync(s->mel_dev.p, ask.mel, (size_t)B1 * mel_floats * 4, hipMemcpyHostToDevice, est));
        mel_dev = s->mel_dev.as<float>();
    }
    const float* mel2_dev = ask.mel2;
    if (pair && !ask.mel2_on_device) {
        float* dst = s->mel_dev.as<float>() + (size_t)B1 * mel_floats;
        HIPCHK(hipMemcpyAsync(dst, ask.mel2, (size_t)B1 * mel_floats * 4, hipMemcpyHostToDevice, est));
        mel2_dev = dst;
    }
    if (score) {
        for (auto& e : s->sc.ev)
            if (!e) HIPCHK(hipEventCreate(&e));
        s->sc.timed = false;
        HIPCHK(hipEventRecord(s->sc.ev[0], est));
    }
    const auto tt0 = std::chrono::steady_clock::now();
    trace_mark(est, "state %p encoder start", (void*)s);
    WMCHK(run_encoder(m, s, mel_dev, pair ? B : n_enc, est, mel2_dev, B1, false));
    trace_mark(est, "state %p encoder end", (void*)s);
    s->enc_stream = est;
    s->has_enc = s->has_cross = true;
    s->last_mel = pair ? nullptr : mel_dev;
    if (wm_env("WM_TRACE_HOST")) {
        const auto tt1 = std::chrono::steady_clock::now();
        (void)hipStreamSynchronize(m->stream);
        fprintf(stderr, "[wm] encoder: enqueue %.3f ms, done after %.3f ms\n", std::chrono::duration<double>(tt1 - tt0).count() * 1e3,
                std::chrono::duration<double>(std::chrono::steady_clock::now() - tt0).count() * 1e3);
    }
    if (lang.only) {  // wm_detect_language: the [sot] pass and the kernel behind the encoder, no transcription
        const wm_state::Lane& ln = s->lanes[0];
        HIPCHK(hipEventRecord(s->enc_done, est));
        HIPCHK(hipStreamWaitEvent(ln.st, s->enc_done, 0));
        WMCHK(lang_pass(m, s, DecView{ln.b0, ln.nb, ln.st, ln.ctl}, nullptr, 0));
        HIPCHK(hipGetLastError());
        s->has_enc = false;  // cache slot 0 holds the [sot] pass: a new wm_encode is needed before wm_decode_step
        return 0;
    }
    if (score) {  // teacher-forced prefill + the vocabulary side on the lane's stream: no loop, no graph, no pump
        s->al.on = false;
        s->shares_chip = !ask.allow_poll;
        WMCHK(score_pass(m, s, *score));
        s->pending = true;
        s->synced = false;
        s->halves_left = 1;
        s->pend_total = score->stride;
        return 0;
    }
    s->al.ragged = false;
    WMCHK(align_setup(m, s, o, cols, ask.win));
    WMCHK(transcribe_decode(m, s, o, ask.allow_poll));
    s->pending = true;
    s->synced = false;
    s->halves_left = pair ? 2 : 1;
    s->pend_total = o->n_prompt + 1 + o->max_loop;
    s->host_len = 0;
    return 0;
}

// Blocks until the state's pending pass is complete, then copies `rows` utterances starting at row0 out.  The pass stays pending
// until every slot that shares the state (one, or the two of a coalesced pair) has collected its rows.
int wait_on(wm_model* m, wm_state* s, int row0, int rows, const PassOut& out) {
    if (!s || !s->pending) return fail(WM_E_STATE, "nothing was submitted on this slot");
    HIPCHK(hipSetDevice(m->device));
    if (rows < 0) rows = s->B;
    if (!s->synced) {
        if (!s->enq_done.load()) {  // the loop pump is still feeding this pass
            std::unique_lock<std::mutex> lk(m->pump_mu);
            m->pump_cv.wait(lk, [&] { return s->enq_done.load(); });
        }
        if (s->enq_rc) {
            s->pending = false;
            for (auto& ln : s->lanes) (void)hipStreamSynchronize(ln.st);
            return fail(s->enq_rc, "%s", s->enq_err.c_str());
        }
        for (auto& ln : s->lanes) HIPCHK(hipEventSynchronize(ln.done));
        s->synced = true;
    }
    const int total = s->pend_total;
    if (out.dev_packed) {  // the gather buffer, built on the device in the caller's DEVICE memory (no host round trip before the collective)
        launch_pack_tokens(s->out_tokens.as<int>() + (size_t)row0 * s->out_stride, s->n_tokens.as<int>() + row0, s->out_stride, rows, out.rows_cap,
                           out.pack_stride, out.dev_packed, s->lanes[0].st);
        HIPCHK(hipGetLastError());
        if (out.dev_times)
            HIPCHK(hipMemcpy2DAsync(out.dev_times, (size_t)out.pack_stride * 4, s->al.times.as<float>() + (size_t)row0 * s->out_stride,
                                    (size_t)s->out_stride * 4, (size_t)total * 4, rows, hipMemcpyDeviceToDevice, s->lanes[0].st));
        HIPCHK(hipStreamSynchronize(s->lanes[0].st));  // the caller's collective runs on another stream
    } else {
        HIPCHK(hipMemcpy2D(out.tokens, (size_t)total * 4, s->out_tokens.as<int>() + (size_t)row0 * s->out_stride, (size_t)s->out_stride * 4, (size_t)total * 4, rows,
                           hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(out.n_tokens, s->n_tokens.as<int>() + row0, (size_t)rows * 4, hipMemcpyDeviceToHost));
        if (out.win_times)  // (the caller's pass was a window pass)
            HIPCHK(hipMemcpy(out.win_times, (const double*)s->al.wtimes.p + (size_t)row0 * (s->al.L + 1), (size_t)rows * (s->al.L + 1) * 8, hipMemcpyDeviceToHost));
        if (out.token_times)
            HIPCHK(hipMemcpy2D(out.token_times, (size_t)total * 4, s->al.times.as<float>() + (size_t)row0 * s->out_stride, (size_t)s->out_stride * 4,
                               (size_t)total * 4, rows, hipMemcpyDeviceToHost));
        if (out.token_logprobs) {  // (the callers checked that the pass computed them)
            HIPCHK(hipMemcpy2D(out.token_logprobs, (size_t)total * 4, s->lp.table.as<float>() + (size_t)row0 * s->out_stride, (size_t)s->out_stride * 4,
                               (size_t)total * 4, rows, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(out.avg_logprob, s->lp.sum.as<float>() + row0, (size_t)rows * 4, hipMemcpyDeviceToHost));
            for (int b = 0; b < rows; ++b) {  // HF _retrieve_avg_logprobs: sum / generated ids (eot included); nothing generated: 0
                const int gen = out.n_tokens[b] - s->lp.n_prompt[row0 + b];
                out.avg_logprob[b] = gen > 0 ? out.avg_logprob[b] / (float)gen : 0.f;
            }
        }
        if (out.no_speech_prob) HIPCHK(hipMemcpy(out.no_speech_prob, s->ns.prob.as<float>() + row0, (size_t)rows * 4, hipMemcpyDeviceToHost));
        if (out.lang_out) HIPCHK(hipMemcpy(out.lang_out, s->lg.out.as<int>() + row0, (size_t)rows * 4, hipMemcpyDeviceToHost));
        if (out.lang_probs)
            HIPCHK(hipMemcpy(out.lang_probs, s->lg.probs.as<float>() + (size_t)row0 * s->lg.n, (size_t)rows * s->lg.n * 4, hipMemcpyDeviceToHost));
    }
    if (--s->halves_left <= 0) {
        s->pending = false;
        s->has_enc = false;  // the KV cache now holds a finished decode: a new wm_encode is needed before wm_decode_step
    }
    return 0;
}

wm_state** slot_state(wm_model* m, int slot) { return slot == 0 ? &m->cached : &m->slots[slot - 1]; }

// ---- the slot protocol: what a slot holds, and the three drivers every entry point ends in -----------------------------
// The one place a SlotRef is filled: the slot holds rows [row0, row0 + rows) of the pass `a`, on state st (null: only held so far).
static void record_pass(wm_model* m, int slot, const PassAsk& a, wm_state* st, int row0, int rows) {
    wm_model::SlotRef& r = m->slot_ref[slot];
    r = wm_model::SlotRef();
    r.pending = true;
    r.st = st;
    r.row0 = row0;
    r.rows = rows;
    r.kind = !a.score ? PassKind::transcribe : a.score->cols ? PassKind::align : a.score->n_utt > 0 ? PassKind::nbest : PassKind::score;
    r.total = a.score ? a.score->stride : a.opts->n_prompt + 1 + a.opts->max_loop;
    r.tt = a.cols != nullptr;
    r.lp = a.score ? a.score->lp : a.lp;
    r.ns = a.ns.token >= 0;
    r.lang = a.lang.ids != nullptr;
}
// Collects the slot's rows and releases the slot.  The one place that says what the slot remembers of a collected pass: the loop
// steps of a transcribe pass, and a reference to the alignment weights of a pass that computed some (token timestamps, or an align
// pass that succeeded) — every other pass clears that reference, for its state's weights are no longer this slot's last pass's.
static int collect_pass(wm_model* m, int slot, const PassOut& out) {
    wm_model::SlotRef& r = m->slot_ref[slot];
    wm_state* s = r.st;
    const bool transcribe = r.kind == PassKind::transcribe;
    const int rc = transcribe ? wait_on(m, s, r.row0, r.rows, out) : score_collect(m, s, out);
    if (!rc && transcribe) m->last_steps[slot] = s->last_steps;
    const bool weights = !rc && (r.tt || r.kind == PassKind::align);
    m->align_ref[slot] = weights ? wm_model::AlignRef{s, r.row0, r.rows, s->al.gen} : wm_model::AlignRef();
    m->topk_ref[slot] = !rc && transcribe && r.lp && s->tk.k > 0 ? wm_model::TopkRef{s, r.row0, r.rows, r.total, s->tk.k, s->tk.gen} : wm_model::TopkRef();
    m->ct_ref[slot] = !rc && transcribe && s->rp.ct ? wm_model::ConstraintRef{s, r.row0, r.rows, s->rp.ct_gen} : wm_model::ConstraintRef();
    r = wm_model::SlotRef();
    return rc;
}

// ---- coalescing of consecutive submits (wm_config.coalesce == 2) ------------------------------------------------------------------
// May this submit share a pass with the held one: the same batch size, outputs asked for and options.
static bool pairs_with(const wm_model::Held& h, const PassAsk& b) {
    const PassAsk& a = h.ask;
    const wm_decode_opts &x = h.o, *o = b.opts;
    if (a.B != b.B || (a.cols != nullptr) != (b.cols != nullptr) || a.lp != b.lp || a.ns.token != b.ns.token || a.ns.n_init != b.ns.n_init)
        return false;
    if (a.top_k != b.top_k) return false;  // one step graph per state: a pair shares the top-k setting
    if (!(a.rp == b.rp)) return false;  // one control block per state: a pair shares (penalty, n-gram size), the sequence-bias table and the constraint's
    if (x.n_prompt != o->n_prompt || x.eot != o->eot || x.max_loop != o->max_loop || x.pos_mode != o->pos_mode || x.ignore_eot != o->ignore_eot ||
        x.n_suppress != (o->suppress_tokens ? o->n_suppress : 0) || x.n_begin_suppress != (o->begin_suppress_tokens ? o->n_begin_suppress : 0) ||
        x.timestamp_begin != o->timestamp_begin || x.no_timestamps_token != o->no_timestamps_token ||
        x.max_initial_timestamp_index != o->max_initial_timestamp_index)
        return false;
    return std::equal(h.prompt.begin(), h.prompt.end(), o->prompt) && std::equal(h.sup.begin(), h.sup.end(), o->suppress_tokens) &&
           std::equal(h.bsup.begin(), h.bsup.end(), o->begin_suppress_tokens);
}
static void hold(wm_model* m, int slot, const PassAsk& a) {
    wm_model::Held& h = m->held;
    const wm_decode_opts* o = a.opts;
    h.active = true;
    h.slot = slot;
    h.prompt.assign(o->prompt, o->prompt + o->n_prompt);
    h.sup.assign(o->suppress_tokens, o->suppress_tokens + (o->suppress_tokens ? o->n_suppress : 0));
    h.bsup.assign(o->begin_suppress_tokens, o->begin_suppress_tokens + (o->begin_suppress_tokens ? o->n_begin_suppress : 0));
    h.cols = a.cols ? *a.cols : std::vector<int32_t>();
    h.o = *o;
    h.o.prompt = h.prompt.data();
    h.o.suppress_tokens = h.sup.empty() ? nullptr : h.sup.data();
    h.o.n_suppress = (int)h.sup.size();
    h.o.begin_suppress_tokens = h.bsup.empty() ? nullptr : h.bsup.data();
    h.o.n_begin_suppress = (int)h.bsup.size();
    h.ask = a;
    h.ask.opts = &h.o;
    h.ask.cols = a.cols ? &h.cols : nullptr;
    record_pass(m, slot, h.ask, nullptr, 0, a.B);
}
// the held submit runs alone, on its own slot's state (no partner came, or the partner did not match)
int flush_held(wm_model* m) {
    wm_model::Held& h = m->held;
    if (!h.active) return 0;
    h.active = false;
    const int rc = submit_on(m, slot_state(m, h.slot), h.ask);
    if (rc) {
        m->slot_ref[h.slot] = wm_model::SlotRef();
        return rc;
    }
    record_pass(m, h.slot, h.ask, *slot_state(m, h.slot), 0, h.ask.B);
    return 0;
}

// ---- the drivers --------------------------------------------------------------------------------------------------------------------
// The synchronous entries run on slot 0.  A held submit goes first: this call may use its mel buffers' stream order, and slot 0.
static int slot0_ready(wm_model* m) {
    WMCHK(flush_held(m));
    if (m->slot_ref[0].pending) return fail(WM_E_STATE, "this slot still holds a pass that was not waited for");
    return 0;
}
// A greedy pass under the model's constraint table: its eot must not be an id of a phrase (the eot is what ends a phrase).  Checked
// before anything is flushed, held or launched.
static int constraint_check(const wm_model* m, const PassAsk& ask) {
    if (!m->repeat.ct || !ask.opts || ask.score || ask.lang.only) return 0;
    if (m->repeat.ct->holds(ask.opts->eot)) return fail(WM_E_ARG, "constraint: a phrase holds the pass's eot %d", ask.opts->eot);
    return 0;
}
int run_now(wm_model* m, PassAsk ask, const PassOut& out) {
    WMCHK(constraint_check(m, ask));
    WMCHK(slot0_ready(m));
    ask.allow_poll = true;
    ask.rp = m->repeat;
    ask.top_k = m->top_k;
    WMCHK(submit_on(m, &m->cached, ask));
    record_pass(m, 0, ask, m->cached, 0, ask.B);
    return collect_pass(m, 0, out);
}
// Pipelined form of Whisper.transcribe for back-to-back batches: submit enqueues the encoder and the greedy loop on the slot's
// stream and returns; the slot's wait blocks until its results are ready.  A pending slot is refused BEFORE a held submit is flushed.
int submit_slot(wm_model* m, int slot, const PassAsk& asked) {
    if (m->slot_ref[slot].pending) return fail(WM_E_STATE, "this slot still holds a pass that was not waited for");
    WMCHK(constraint_check(m, asked));
    PassAsk ask = asked;
    ask.rp = m->repeat;  // the setting in force now: a held submit runs with it even if it changes before the partner arrives
    ask.top_k = m->top_k;
    const int B = ask.B;
    // (a per-row, language or score / align pass is never held for a coalesce = 2 partner: it runs alone)
    const bool can_pair = !ask.rows && !ask.lang.ids && !ask.score && m->cfg.coalesce == 2 && B <= m->cfg.max_batch &&
                          (B <= m->enc_chunk || B % m->enc_chunk == 0);
    if (can_pair && m->held.active && pairs_with(m->held, ask)) {
        // the partner of the held submit: both batches go out as ONE pass on a 2·B-row state
        wm_state** ps = nullptr;
        for (auto& pr : m->pairs)
            if (pr && !pr->pending && pr->B == 2 * B) ps = &pr;
        for (auto& pr : m->pairs)
            if (!ps && !pr) ps = &pr;
        for (auto& pr : m->pairs)
            if (!ps && !pr->pending) ps = &pr;  // another batch size: re-created
        if (ps) {
            wm_model::Held& h = m->held;
            h.active = false;
            PassAsk both = h.ask;
            both.B = 2 * B;
            both.mel2 = ask.mel;
            both.mel2_on_device = ask.mel_on_device;
            std::vector<int32_t> pair_cols;
            if (ask.cols) {  // rows [0, B) are the held batch's, [B, 2B) this one's
                pair_cols = h.cols;
                pair_cols.insert(pair_cols.end(), ask.cols->begin(), ask.cols->end());
                both.cols = &pair_cols;
            }
            const int rc = submit_on(m, ps, both);
            if (rc) {
                m->slot_ref[h.slot] = wm_model::SlotRef();
                return rc;
            }
            record_pass(m, h.slot, h.ask, *ps, 0, B);
            record_pass(m, slot, ask, *ps, B, B);
            return 0;
        }
    }
    WMCHK(flush_held(m));
    if (can_pair) {  // wait for a partner (or for this slot's wait)
        hold(m, slot, ask);
        return 0;
    }
    WMCHK(submit_on(m, slot_state(m, slot), ask));
    record_pass(m, slot, ask, *slot_state(m, slot), 0, B);
    return 0;
}
// A wait of the `kind` family on a slot: refused (the pass stays pending, collectable by the right wait) when the slot holds another
// kind of pass or one submitted without something `out` asks for.
int collect_slot(wm_model* m, int slot, PassKind kind, const PassOut& out) {
    const wm_model::SlotRef& r = m->slot_ref[slot];
    if (!r.pending) return fail(WM_E_STATE, "nothing was submitted on this slot");
    if (r.kind != kind) {
        if (r.kind == PassKind::score) return fail(WM_E_STATE, "this slot holds a score pass (collect it with wm_score_wait)");
        if (r.kind == PassKind::nbest) return fail(WM_E_STATE, "this slot holds an n-best score pass (collect it with wm_score_nbest_wait)");
        if (r.kind == PassKind::align) return fail(WM_E_STATE, "this slot holds an align pass (collect it with wm_align_wait)");
        return fail(WM_E_STATE, "this slot holds a transcribe pass (collect it with wm_transcribe_wait)");
    }
    if (kind == PassKind::align) {
        if (out.token_logprobs && !r.lp) return fail(WM_E_STATE, "this slot's align pass was submitted without log-probabilities");
    } else if (kind == PassKind::transcribe) {
        if (out.lang_out && !r.lang) return fail(WM_E_STATE, "this slot's pass was submitted without language detection (wm_transcribe_submit_lang)");
        if (out.no_speech_prob && !r.ns) return fail(WM_E_STATE, "this slot's pass was submitted without the no-speech probe (wm_transcribe_submit_lp_ns)");
        if (out.token_logprobs && !r.lp) return fail(WM_E_STATE, "this slot's pass was submitted without log-probabilities (wm_transcribe_submit_lp)");
        if ((out.token_times || out.dev_times) && !r.tt)
            return fail(WM_E_STATE, "this slot's pass was submitted without token timestamps (wm_transcribe_submit_tt)");
        if (out.dev_packed && out.rows_cap < r.rows) return fail(WM_E_ARG, "rows_cap %d is smaller than the batch (%d)", out.rows_cap, r.rows);
        if (out.dev_packed && out.pack_stride < r.total)
            return fail(WM_E_ARG, "stride %d is smaller than the pass's ids per utterance (%d)", out.pack_stride, r.total);
    }
    if (m->held.active && m->held.slot == slot) WMCHK(flush_held(m));  // no partner came: the held batch runs alone now
    return collect_pass(m, slot, out);
}

// n_frames -> columns kept per row (HF crops the attentions to n_frames // 2 encoder positions); null = every column
int align_cols(wm_model* m, const int32_t* n_frames, int B, std::vector<int32_t>& cols) {
    const int T = m->cfg.dims.n_audio_ctx;
    if (m->align_pairs.empty()) return fail(WM_E_STATE, "token timestamps need alignment heads (wm_set_alignment_heads)");
    cols.assign(B, T);
    if (n_frames)
        for (int b = 0; b < B; ++b) {
            if (n_frames[b] < 2 || n_frames[b] > 2 * T)
                return fail(WM_E_ARG, "n_frames[%d] = %d: must lie in [2, %d] (mel frames of real audio)", b, n_frames[b], 2 * T);
            cols[b] = n_frames[b] / 2;
        }
    return 0;
}

extern "C" int wm_transcribe(wm_model* m, const float* mel, int mel_on_device, int B, const wm_decode_opts* o,
                             int32_t* tokens_out, int32_t* n_tokens) {
    if (!m || !mel || !tokens_out || !n_tokens) return fail(WM_E_ARG, "bad argument");
    WMCHK(check_opts(m, o, B));
    return run_now(m, PassAsk{mel, mel_on_device, B, o}, PassOut{tokens_out, n_tokens});
}

extern "C" int wm_transcribe_tt(wm_model* m, const float* mel, int mel_on_device, int B, const wm_decode_opts* o, const int32_t* n_frames,
                                int32_t* tokens_out, int32_t* n_tokens, float* token_times) {
    if (!m || !mel || !tokens_out || !n_tokens || !token_times) return fail(WM_E_ARG, "bad argument");
    WMCHK(check_opts(m, o, B));
    std::vector<int32_t> cols;
    WMCHK(align_cols(m, n_frames, B, cols));
    PassAsk ask{mel, mel_on_device, B, o};
    ask.cols = &cols;
    return run_now(m, ask, PassOut{tokens_out, n_tokens, token_times});
}

extern "C" int wm_transcribe_submit(wm_model* m, int slot, const float* mel, int mel_on_device, int B, const wm_decode_opts* o) {
    if (!m || !mel || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument (slot must be 0..7)");
    WMCHK(check_opts(m, o, B));
    return submit_slot(m, slot, PassAsk{mel, mel_on_device, B, o});
}
extern "C" int wm_transcribe_submit_tt(wm_model* m, int slot, const float* mel, int mel_on_device, int B, const wm_decode_opts* o,
                                       const int32_t* n_frames) {
    if (!m || !mel || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument (slot must be 0..7)");
    WMCHK(check_opts(m, o, B));
    std::vector<int32_t> cols;
    WMCHK(align_cols(m, n_frames, B, cols));
    PassAsk ask{mel, mel_on_device, B, o};
    ask.cols = &cols;
    return submit_slot(m, slot, ask);
}
// ---- per-row prompts -----------------------------------------------------------------------------------------------
// Everything is checked before anything is launched.  o2: the options the pass runs with (n_prompt = the longest row).
int rows_check(wm_model* m, const wm_decode_opts* o, int B, const int32_t* prompts, const int32_t* prompt_len, int prompt_stride,
                      wm_decode_opts& o2, RowPrompts& rows) {
    if (!o || B <= 0 || !prompts || !prompt_len || prompt_stride <= 0) return fail(WM_E_ARG, "bad argument");
    o2 = *o;
    o2.prompt = prompts;  // (ignored by a per-row pass; the generic checks want one valid id)
    o2.n_prompt = 1;
    const wm_dims& c = m->cfg.dims;
    int Lmax = 0;
    for (int b = 0; b < B; ++b) {
        const int L = prompt_len[b];
        if (L < 1 || L > prompt_stride) return fail(WM_E_ARG, "prompt_len[%d] = %d outside [1, prompt_stride = %d]", b, L, prompt_stride);
        for (int i = 0; i < L; ++i) {
            const int32_t id = prompts[(size_t)b * prompt_stride + i];
            if (id < 0 || id >= c.vocab) return fail(WM_E_ARG, "prompt id %d of row %d out of range", id, b);
        }
        Lmax = std::max(Lmax, L);
    }
    WMCHK(check_opts(m, &o2, B));
    if (dec_lanes_for(B) != 1) return fail(WM_E_ARG, "per-row prompts need a single-lane decode state");
    if (o->max_loop < 0 || Lmax + 1 + o->max_loop > c.n_text_ctx)
        return fail(WM_E_ARG, "longest prompt %d + 1 + max_loop %d exceeds the decoder context %d", Lmax, o->max_loop, c.n_text_ctx);
    o2.n_prompt = Lmax;
    rows = RowPrompts{prompts, prompt_len, prompt_stride, Lmax};
    return 0;
}
extern "C" int wm_transcribe_rows(wm_model* m, const float* mel, int mel_on_device, int B, const wm_decode_opts* o, const int32_t* prompts,
                                  const int32_t* prompt_len, int prompt_stride, int32_t* tokens_out, int32_t* n_tokens) {
    if (!m || !mel || !tokens_out || !n_tokens) return fail(WM_E_ARG, "bad argument");
    wm_decode_opts o2;
    RowPrompts rows;
    WMCHK(rows_check(m, o, B, prompts, prompt_len, prompt_stride, o2, rows));
    PassAsk ask{mel, mel_on_device, B, &o2};
    ask.rows = &rows;
    return run_now(m, ask, PassOut{tokens_out, n_tokens});
}
extern "C" int wm_transcribe_submit_rows(wm_model* m, int slot, const float* mel, int mel_on_device, int B, const wm_decode_opts* o,
                                         const int32_t* prompts, const int32_t* prompt_len, int prompt_stride) {
    if (!m || !mel || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument (slot must be 0..7)");
    wm_decode_opts o2;
    RowPrompts rows;
    WMCHK(rows_check(m, o, B, prompts, prompt_len, prompt_stride, o2, rows));
    PassAsk ask{mel, mel_on_device, B, &o2};
    ask.rows = &rows;
    return submit_slot(m, slot, ask);
}
extern "C" int wm_transcribe_wait(wm_model* m, int slot, int32_t* tokens_out, int32_t* n_tokens) {
    if (!m || !tokens_out || !n_tokens || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument");
    return collect_slot(m, slot, PassKind::transcribe, PassOut{tokens_out, n_tokens});
}
extern "C" int wm_transcribe_wait_tt(wm_model* m, int slot, int32_t* tokens_out, int32_t* n_tokens, float* token_times) {
    if (!m || !tokens_out || !n_tokens || !token_times || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument");
    return collect_slot(m, slot, PassKind::transcribe, PassOut{tokens_out, n_tokens, token_times});
}
// ---- log-probabilities -----------------------------------------------------------------------------------------------
// One family for shared (prompts == NULL: opts->prompt) and per-row prompts.  Everything is refused before anything is launched.
static int lp_check(wm_model* m, const wm_decode_opts* o, int B, const int32_t* prompts, const int32_t* prompt_len, int prompt_stride,
                    wm_decode_opts& o2, RowPrompts& rows) {
    if (prompts) {
        WMCHK(rows_check(m, o, B, prompts, prompt_len, prompt_stride, o2, rows));
    } else {
        if (prompt_len) return fail(WM_E_ARG, "prompt_len without prompts");
        WMCHK(check_opts(m, o, B));
        o2 = *o;
    }
    if (dec_lanes_for(B) != 1) return fail(WM_E_ARG, "log-probabilities need a single-lane decode state");
    return 0;
}
static int ns_check(wm_model* m, const wm_decode_opts& o2, int B, const int32_t* prompts, const int32_t* prompt_len, int no_speech_token, int n_init) {
    if (no_speech_token < 0 || no_speech_token >= m->cfg.dims.vocab) return fail(WM_E_ARG, "no_speech_token %d is not a vocabulary id", no_speech_token);
    if (n_init < 1) return fail(WM_E_ARG, "n_init must be >= 1 (the initial ids start at <|startoftranscript|>)");
    if (prompts) {
        for (int b = 0; b < B; ++b)
            if (n_init > prompt_len[b]) return fail(WM_E_ARG, "n_init %d exceeds prompt_len[%d] = %d", n_init, b, prompt_len[b]);
    } else if (n_init > o2.n_prompt) {
        return fail(WM_E_ARG, "n_init %d exceeds the prompt length %d", n_init, o2.n_prompt);
    }
    return 0;
}
// The _lp and _lp_ns entries behind their null checks: slot < 0 runs the pass now, on slot 0; ns: the _lp_ns probe, as given.
static int lp_entry(wm_model* m, int slot, const float* mel, int mel_on_device, int B, const wm_decode_opts* o, const int32_t* prompts,
                    const int32_t* prompt_len, int prompt_stride, const NsAsk* ns, const PassOut& out) {
    wm_decode_opts o2;
    RowPrompts rows;
    WMCHK(lp_check(m, o, B, prompts, prompt_len, prompt_stride, o2, rows));
    if (ns) WMCHK(ns_check(m, o2, B, prompts, prompt_len, ns->token, ns->n_init));
    PassAsk ask{mel, mel_on_device, B, &o2};
    ask.rows = prompts ? &rows : nullptr;
    ask.lp = true;
    if (ns) ask.ns = *ns;
    return slot < 0 ? run_now(m, ask, out) : submit_slot(m, slot, ask);
}
static PassOut lp_out(int32_t* tokens_out, int32_t* n_tokens, float* token_logprobs, float* avg_logprob, float* no_speech_prob) {
    PassOut out{tokens_out, n_tokens};
    out.token_logprobs = token_logprobs;
    out.avg_logprob = avg_logprob;
    out.no_speech_prob = no_speech_prob;
    return out;
}
extern "C" int wm_transcribe_lp(wm_model* m, const float* mel, int mel_on_device, int B, const wm_decode_opts* o, const int32_t* prompts,
                                const int32_t* prompt_len, int prompt_stride, int32_t* tokens_out, int32_t* n_tokens, float* token_logprobs,
                                float* avg_logprob) {
    if (!m || !mel || !tokens_out || !n_tokens || !token_logprobs || !avg_logprob) return fail(WM_E_ARG, "bad argument");
    return lp_entry(m, -1, mel, mel_on_device, B, o, prompts, prompt_len, prompt_stride, nullptr,
                    lp_out(tokens_out, n_tokens, token_logprobs, avg_logprob, nullptr));
}
extern "C" int wm_transcribe_submit_lp(wm_model* m, int slot, const float* mel, int mel_on_device, int B, const wm_decode_opts* o,
                                       const int32_t* prompts, const int32_t* prompt_len, int prompt_stride) {
    if (!m || !mel || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument (slot must be 0..7)");
    return lp_entry(m, slot, mel, mel_on_device, B, o, prompts, prompt_len, prompt_stride, nullptr, PassOut());
}
extern "C" int wm_transcribe_wait_lp(wm_model* m, int slot, int32_t* tokens_out, int32_t* n_tokens, float* token_logprobs, float* avg_logprob) {
    if (!m || !tokens_out || !n_tokens || !token_logprobs || !avg_logprob || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument");
    return collect_slot(m, slot, PassKind::transcribe, lp_out(tokens_out, n_tokens, token_logprobs, avg_logprob, nullptr));
}
// ---- no-speech probe: the _lp trio plus the probability of no_speech_token at each row's <|startoftranscript|>
// position, prompt length - n_init.  Everything is refused before anything is launched.
extern "C" int wm_transcribe_lp_ns(wm_model* m, const float* mel, int mel_on_device, int B, const wm_decode_opts* o, const int32_t* prompts,
                                   const int32_t* prompt_len, int prompt_stride, int no_speech_token, int n_init, int32_t* tokens_out,
                                   int32_t* n_tokens, float* token_logprobs, float* avg_logprob, float* no_speech_prob) {
    if (!m || !mel || !tokens_out || !n_tokens || !token_logprobs || !avg_logprob || !no_speech_prob) return fail(WM_E_ARG, "bad argument");
    const NsAsk ns{no_speech_token, n_init};
    return lp_entry(m, -1, mel, mel_on_device, B, o, prompts, prompt_len, prompt_stride, &ns,
                    lp_out(tokens_out, n_tokens, token_logprobs, avg_logprob, no_speech_prob));
}
extern "C" int wm_transcribe_submit_lp_ns(wm_model* m, int slot, const float* mel, int mel_on_device, int B, const wm_decode_opts* o,
                                          const int32_t* prompts, const int32_t* prompt_len, int prompt_stride, int no_speech_token, int n_init) {
    if (!m || !mel || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument (slot must be 0..7)");
    const NsAsk ns{no_speech_token, n_init};
    return lp_entry(m, slot, mel, mel_on_device, B, o, prompts, prompt_len, prompt_stride, &ns, PassOut());
}
extern "C" int wm_transcribe_wait_lp_ns(wm_model* m, int slot, int32_t* tokens_out, int32_t* n_tokens, float* token_logprobs, float* avg_logprob,
                                        float* no_speech_prob) {
    if (!m || !tokens_out || !n_tokens || !token_logprobs || !avg_logprob || !no_speech_prob || slot < 0 || slot >= wm_model::NSLOT)
        return fail(WM_E_ARG, "bad argument");
    return collect_slot(m, slot, PassKind::transcribe, lp_out(tokens_out, n_tokens, token_logprobs, avg_logprob, no_speech_prob));
}
// ---- language detection ----------------------------------------------------------------------------------------------
// Everything is refused before anything is launched.
int lang_list_check(int vocab, const int32_t* lang_ids, int n_lang) {
    if (n_lang < 1 || n_lang > LANG_DETECT_MAX) return fail(WM_E_ARG, "n_lang = %d outside [1, %d]", n_lang, LANG_DETECT_MAX);
    if (!lang_ids) return fail(WM_E_ARG, "bad argument");
    for (int i = 0; i < n_lang; ++i) {
        if (lang_ids[i] < 0 || lang_ids[i] >= vocab) return fail(WM_E_ARG, "language id %d is not a vocabulary id", lang_ids[i]);
        for (int j = 0; j < i; ++j)
            if (lang_ids[j] == lang_ids[i]) return fail(WM_E_ARG, "language id %d is listed twice", lang_ids[i]);
    }
    return 0;
}
// (the synchronous sequence up to the submit; the collect is its own: no ids, and the pass leaves no pending state behind)
extern "C" int wm_detect_language(wm_model* m, const float* mel, int mel_on_device, int B, int sot_token, const int32_t* lang_ids, int n_lang,
                                  int32_t* lang_out, float* probs_out) {
    if (!m || !mel || !lang_out || B <= 0) return fail(WM_E_ARG, "bad argument");
    if (B > m->cfg.max_batch) return fail(WM_E_ARG, "B = %d exceeds max_batch %d", B, m->cfg.max_batch);
    if (sot_token < 0 || sot_token >= m->cfg.dims.vocab) return fail(WM_E_ARG, "sot_token %d is not a vocabulary id", sot_token);
    WMCHK(lang_list_check(m->cfg.dims.vocab, lang_ids, n_lang));
    if (dec_lanes_for(B) != 1) return fail(WM_E_ARG, "language detection needs a single-lane decode state");
    WMCHK(slot0_ready(m));
    WMCHK(submit_on(m, &m->cached, lang_only_ask(mel, mel_on_device, B, lang_ids, n_lang, sot_token)));
    wm_state* s = m->cached;
    HIPCHK(hipStreamSynchronize(s->lanes[0].st));
    HIPCHK(hipMemcpy(lang_out, s->lg.out.p, (size_t)B * 4, hipMemcpyDeviceToHost));
    if (probs_out) HIPCHK(hipMemcpy(probs_out, s->lg.probs.p, (size_t)B * n_lang * 4, hipMemcpyDeviceToHost));
    return 0;
}
// The _lang entries behind their null checks: the checks of a _lang pass, then slot < 0 runs it now, on slot 0.
int lang_entry(wm_model* m, int slot, const float* mel, int mel_on_device, int B, const wm_decode_opts* o, const int32_t* prompts,
                      const int32_t* prompt_len, int prompt_stride, bool lp, int no_speech_token, int n_init, const int32_t* lang_ids, int n_lang,
                      const PassOut& out) {
    std::vector<int32_t> tab, len;  // the per-row table built from opts->prompt when prompts == NULL
    wm_decode_opts o2;
    RowPrompts rows;
    if (!prompts) {
        if (prompt_len) return fail(WM_E_ARG, "prompt_len without prompts");
        WMCHK(check_opts(m, o, B));
        tab.resize((size_t)B * o->n_prompt);
        for (int b = 0; b < B; ++b) std::copy(o->prompt, o->prompt + o->n_prompt, tab.begin() + (size_t)b * o->n_prompt);
        len.assign(B, o->n_prompt);
        prompts = tab.data();
        prompt_len = len.data();
        prompt_stride = o->n_prompt;
    }
    WMCHK(rows_check(m, o, B, prompts, prompt_len, prompt_stride, o2, rows));  // (single lane included)
    if (no_speech_token >= 0) {
        if (!lp) return fail(WM_E_ARG, "the no-speech probe needs the log-prob outputs");
        WMCHK(ns_check(m, o2, B, prompts, prompt_len, no_speech_token, n_init));
    }
    WMCHK(lang_list_check(m->cfg.dims.vocab, lang_ids, n_lang));
    if (n_init < 2) return fail(WM_E_ARG, "n_init must be >= 2 (<|startoftranscript|> and the language slot)");
    const int32_t sot = prompts[prompt_len[0] - n_init >= 0 ? prompt_len[0] - n_init : 0];
    for (int b = 0; b < B; ++b) {
        if (n_init > prompt_len[b]) return fail(WM_E_ARG, "n_init %d exceeds prompt_len[%d] = %d", n_init, b, prompt_len[b]);
        if (prompts[(size_t)b * prompt_stride + prompt_len[b] - n_init] != sot)
            return fail(WM_E_ARG, "row %d starts its initial ids with %d, row 0 with %d: one <|startoftranscript|> per pass", b,
                        prompts[(size_t)b * prompt_stride + prompt_len[b] - n_init], sot);
    }
    PassAsk ask{mel, mel_on_device, B, &o2};
    ask.rows = &rows;
    ask.lp = lp;
    if (no_speech_token >= 0) ask.ns = NsAsk{no_speech_token, n_init};
    ask.lang.ids = lang_ids;
    ask.lang.n = n_lang;
    ask.lang.n_init = n_init;
    ask.lang.sot = sot;
    return slot < 0 ? run_now(m, ask, out) : submit_slot(m, slot, ask);
}
extern "C" int wm_transcribe_lang(wm_model* m, const float* mel, int mel_on_device, int B, const wm_decode_opts* o, const int32_t* prompts,
                                  const int32_t* prompt_len, int prompt_stride, int no_speech_token, int n_init, const int32_t* lang_ids, int n_lang,
                                  int32_t* tokens_out, int32_t* n_tokens, float* token_logprobs, float* avg_logprob, float* no_speech_prob,
                                  int32_t* lang_out, float* lang_probs) {
    if (!m || !mel || !tokens_out || !n_tokens || !lang_out || !o || B <= 0) return fail(WM_E_ARG, "bad argument");
    if (!token_logprobs != !avg_logprob) return fail(WM_E_ARG, "token_logprobs and avg_logprob go together");
    if (no_speech_token >= 0 && !no_speech_prob) return fail(WM_E_ARG, "bad argument");
    PassOut out = lp_out(tokens_out, n_tokens, token_logprobs, avg_logprob, no_speech_token >= 0 ? no_speech_prob : nullptr);
    out.lang_out = lang_out;
    out.lang_probs = lang_probs;
    return lang_entry(m, -1, mel, mel_on_device, B, o, prompts, prompt_len, prompt_stride, token_logprobs != nullptr, no_speech_token, n_init, lang_ids,
                      n_lang, out);
}
extern "C" int wm_transcribe_submit_lang(wm_model* m, int slot, const float* mel, int mel_on_device, int B, const wm_decode_opts* o,
                                         const int32_t* prompts, const int32_t* prompt_len, int prompt_stride, int no_speech_token, int n_init,
                                         const int32_t* lang_ids, int n_lang, int want_logprobs) {
    if (!m || !mel || !o || B <= 0 || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument (slot must be 0..7)");
    return lang_entry(m, slot, mel, mel_on_device, B, o, prompts, prompt_len, prompt_stride, want_logprobs != 0, no_speech_token, n_init, lang_ids,
                      n_lang, PassOut());
}
extern "C" int wm_transcribe_wait_lang(wm_model* m, int slot, int32_t* tokens_out, int32_t* n_tokens, float* token_logprobs, float* avg_logprob,
                                       float* no_speech_prob, int32_t* lang_out, float* lang_probs) {
    if (!m || !tokens_out || !n_tokens || !lang_out || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument");
    if (!token_logprobs != !avg_logprob) return fail(WM_E_ARG, "token_logprobs and avg_logprob go together");
    PassOut out = lp_out(tokens_out, n_tokens, token_logprobs, avg_logprob, no_speech_prob);
    out.lang_out = lang_out;
    out.lang_probs = lang_probs;
    return collect_slot(m, slot, PassKind::transcribe, out);
}
// ---- repetition processors -------------------------------------------------------------------------------------
extern "C" int wm_set_repeat_options(wm_model* m, float repetition_penalty, int no_repeat_ngram_size) {
    if (!m) return fail(WM_E_ARG, "bad argument");
    if (!(repetition_penalty > 0.f) || !std::isfinite(repetition_penalty))
        return fail(WM_E_ARG, "repetition_penalty must be a finite float > 0 (1 = off)");
    if (no_repeat_ngram_size < 0 || no_repeat_ngram_size > REPEAT_NGRAM_MAX)
        return fail(WM_E_ARG, "no_repeat_ngram_size %d outside [0, %d] (0 = off)", no_repeat_ngram_size, REPEAT_NGRAM_MAX);
    m->repeat.penalty = repetition_penalty;
    m->repeat.ngram = no_repeat_ngram_size;
    return 0;
}
// ---- phrase-list constraint ----------------------------------------------------------------------------------------
// Validates the phrases, builds their trie and flattens it to CSR on the device.  Nodes are numbered in the order the phrases, taken
// in the caller's order and id by id, first reach them; the root is 0 and the dead node comes last.  Nothing is allocated before every
// argument has passed.  free_from < 0 or >= vocab: no free ids.
int build_constraint_table(std::shared_ptr<ConstraintTable>& out, int vocab, const int32_t* ids, const int32_t* off, int n_phrases, int free_from) {
    if (n_phrases < 0 || (n_phrases > 0 && (!ids || !off))) return fail(WM_E_ARG, "bad argument");
    out.reset();
    if (n_phrases == 0) return 0;
    if (n_phrases > CONSTRAINT_PHRASES_MAX) return fail(WM_E_ARG, "constraint: %d phrases, at most %d", n_phrases, CONSTRAINT_PHRASES_MAX);
    if (off[0] != 0) return fail(WM_E_ARG, "constraint: offsets start at 0");
    const int ff = free_from < 0 || free_from > vocab ? vocab : free_from;
    std::vector<std::vector<std::pair<int32_t, int32_t>>> kids(1);  // per node: (id, child), kept ascending by id
    std::vector<int32_t> term(1, -1);
    for (int q = 0; q < n_phrases; ++q) {
        const long long len = (long long)off[q + 1] - off[q];
        if (len < 1 || len > CONSTRAINT_LEN_MAX) return fail(WM_E_ARG, "constraint: phrase %d has %lld ids, need 1..%d", q, len, CONSTRAINT_LEN_MAX);
        int v = 0;
        for (int k = 0; k < (int)len; ++k) {
            const int32_t t = ids[off[q] + k];
            if (t < 0 || t >= vocab) return fail(WM_E_ARG, "constraint: phrase %d holds id %d outside the vocabulary of %d", q, t, vocab);
            if (t >= ff) return fail(WM_E_ARG, "constraint: phrase %d holds the free id %d (free_from %d)", q, t, ff);
            auto& e = kids[v];
            auto it = std::lower_bound(e.begin(), e.end(), std::make_pair(t, (int32_t)-1));
            if (it != e.end() && it->first == t) {
                v = it->second;
            } else {
                if ((long long)kids.size() + 2 > CONSTRAINT_NODES_MAX)
                    return fail(WM_E_ARG, "constraint: more than %d trie nodes", CONSTRAINT_NODES_MAX);
                const int32_t nv = (int32_t)kids.size();
                e.insert(it, std::make_pair(t, nv));  // (kids grows below: e is not used again)
                kids.emplace_back();
                term.push_back(-1);
                v = nv;
            }
        }
        if (term[v] >= 0) return fail(WM_E_ARG, "constraint: phrase %d is a duplicate of phrase %d", q, term[v]);
        term[v] = q;
    }
    kids.emplace_back();  // the dead node
    term.push_back(-1);
    std::vector<int32_t> h_off{0}, h_id, h_next;
    for (const auto& e : kids) {
        for (const auto& pr : e) {
            h_id.push_back(pr.first);
            h_next.push_back(pr.second);
        }
        h_off.push_back((int32_t)h_id.size());
    }
    auto t = std::make_shared<ConstraintTable>();
    (void)hipGetDevice(&t->device);  // (the callers have made the model's device current)
    t->n_nodes = (int)kids.size();
    t->dead = t->n_nodes - 1;
    t->n_phrases = n_phrases;
    t->free_from = ff;
    t->ids = h_id;
    std::sort(t->ids.begin(), t->ids.end());
    t->ids.erase(std::unique(t->ids.begin(), t->ids.end()), t->ids.end());
    WMCHK(upload_bytes(t->edge_off, h_off.data(), h_off.size() * 4));
    WMCHK(upload_bytes(t->edge_id, h_id.data(), h_id.size() * 4));
    WMCHK(upload_bytes(t->edge_next, h_next.data(), h_next.size() * 4));
    WMCHK(upload_bytes(t->terminal, term.data(), term.size() * 4));
    out = std::move(t);
    return 0;
}
extern "C" int wm_set_constraint(wm_model* m, const int32_t* ids, const int32_t* offsets, int n_phrases, int free_from) {
    if (!m) return fail(WM_E_ARG, "bad argument");
    if (n_phrases == 0 && ids) return fail(WM_E_ARG, "constraint: an empty list of phrases (pass NULL to switch the constraint off)");
    HIPCHK(hipSetDevice(m->device));
    std::shared_ptr<ConstraintTable> t;
    WMCHK(build_constraint_table(t, m->cfg.dims.vocab, ids, offsets, n_phrases, free_from));
    if (t) t->gen = ++m->ct_gen;
    m->repeat.ct = std::move(t);  // a held submit and a pending pass keep the table they were asked for with
    return 0;
}
extern "C" int wm_transcribe_constraint_match(wm_model* m, int slot, int32_t* out, int B) {
    if (!m || !out || slot < 0 || slot > 7) return fail(WM_E_ARG, "bad argument");
    const wm_model::ConstraintRef& r = m->ct_ref[slot];
    if (!r.st || !state_is_live(r.st) || r.st->rp.ct_gen != r.gen)
        return fail(WM_E_STATE, "no collected pass under a constraint on this slot (wm_set_constraint; or its state has run another pass since)");
    if (B != r.rows) return fail(WM_E_ARG, "constraint_match: the pass had %d rows, not %d", r.rows, B);
    HIPCHK(hipSetDevice(m->device));
    HIPCHK(hipMemcpy(out, r.st->rp.match.as<int>() + r.row0, (size_t)B * 4, hipMemcpyDeviceToHost));
    return 0;
}
// ---- top-k alternatives ----------------------------------------------------------------------------------------
extern "C" int wm_set_top_k(wm_model* m, int top_k) {
    if (!m) return fail(WM_E_ARG, "bad argument");
    if (top_k < 0 || top_k > TOPK_MAX) return fail(WM_E_ARG, "top_k %d outside [0, %d] (0 = off)", top_k, TOPK_MAX);
    m->top_k = top_k;
    return 0;
}
extern "C" int wm_transcribe_top_k(wm_model* m, int slot, int32_t* top_ids, float* top_logprobs) {
    if (!m || !top_ids || !top_logprobs || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument");
    const wm_model::TopkRef& r = m->topk_ref[slot];
    if (!r.st || !state_is_live(r.st) || r.st->tk.gen != r.gen || (r.st->pending && r.st->synced == false))
        return fail(WM_E_STATE, "no collected log-prob pass with top_k on this slot (wm_set_top_k; or its state has run another pass since)");
    wm_state* s = r.st;
    HIPCHK(hipSetDevice(m->device));
    const size_t k = r.k, row = (size_t)r.total * k, pitch = (size_t)s->out_stride * k;
    HIPCHK(hipMemcpy2D(top_ids, row * 4, s->tk.ids.as<int>() + (size_t)r.row0 * pitch, pitch * 4, row * 4, r.rows, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy2D(top_logprobs, row * 4, s->tk.lps.as<float>() + (size_t)r.row0 * pitch, pitch * 4, row * 4, r.rows, hipMemcpyDeviceToHost));
    std::vector<int32_t> n(r.rows);
    HIPCHK(hipMemcpy(n.data(), s->n_tokens.as<int>() + r.row0, (size_t)r.rows * 4, hipMemcpyDeviceToHost));
    for (int b = 0; b < r.rows; ++b)  // prompt and tail positions were never written: id -1, log-prob 0, as the log-prob table's 0
        for (int i = 0; i < r.total; ++i)
            if (i < s->lp.n_prompt[r.row0 + b] || i >= n[b])
                for (size_t j = 0; j < k; ++j) {
                    top_ids[b * row + i * k + j] = -1;
                    top_logprobs[b * row + i * k + j] = 0.f;
                }
    return 0;
}
// ---- sequence bias and bad words ---------------------------------------------------------------------------------
// Validates both lists and builds the device table: the sequences grouped by last id (ascending), inside a group the length-1 bias
// first, then the bias sequences in the caller's order, then the bans — the order one thread sums a group in.  Nothing is allocated
// before every argument has passed.  slot_ids (optional): the groups' ids for the op hook.
int build_seq_table(std::shared_ptr<SeqTable>& out, int vocab, const int32_t* ids, const int32_t* off, const float* bias, int n_seq,
                    const int32_t* bad_ids, const int32_t* bad_off, int n_bad, std::vector<int32_t>* slot_ids) {
    if (n_seq < 0 || n_bad < 0 || (n_seq > 0 && (!ids || !off || !bias)) || (n_bad > 0 && (!bad_ids || !bad_off))) return fail(WM_E_ARG, "bad argument");
    if ((long long)n_seq + n_bad > SEQ_BIAS_MAX) return fail(WM_E_ARG, "%d + %d sequences: at most %d over the two lists", n_seq, n_bad, SEQ_BIAS_MAX);
    struct Ent {
        const int32_t* p;
        int len, ban, order;
        float bias;
    };
    std::vector<Ent> es;
    for (int list = 0; list < 2; ++list) {
        const int n = list ? n_bad : n_seq;
        const int32_t *id = list ? bad_ids : ids, *o = list ? bad_off : off;
        const char* what = list ? "bad_words_ids" : "sequence_bias";
        std::set<std::vector<int32_t>> had;
        if (n > 0 && o[0] != 0) return fail(WM_E_ARG, "%s: offsets start at 0", what);
        for (int q = 0; q < n; ++q) {
            const long long len = (long long)o[q + 1] - o[q];
            if (len < 1 || len > SEQ_BIAS_LEN_MAX) return fail(WM_E_ARG, "%s: sequence %d has %lld ids, need 1..%d", what, q, len, SEQ_BIAS_LEN_MAX);
            for (int k = 0; k < (int)len; ++k)
                if (id[o[q] + k] < 0 || id[o[q] + k] >= vocab) return fail(WM_E_ARG, "%s: sequence %d holds id %d outside the vocabulary of %d", what, q, id[o[q] + k], vocab);
            if (!had.insert(std::vector<int32_t>(id + o[q], id + o[q + 1])).second) return fail(WM_E_ARG, "%s: sequence %d is a duplicate", what, q);
            if (!list && !(std::isfinite(bias[q]) || (std::isinf(bias[q]) && bias[q] < 0.f)))
                return fail(WM_E_ARG, "sequence_bias: the bias of sequence %d must be a finite float or -inf", q);
            es.push_back(Ent{id + o[q], (int)len, list, (int)es.size(), list ? -INFINITY : bias[q]});
        }
    }
    out.reset();
    if (es.empty()) return 0;
    std::sort(es.begin(), es.end(), [](const Ent& a, const Ent& b) {
        const int la = a.p[a.len - 1], lb = b.p[b.len - 1];
        if (la != lb) return la < lb;
        if (a.ban != b.ban) return a.ban < b.ban;
        const int ra = !a.ban && a.len == 1 ? 0 : 1, rb = !b.ban && b.len == 1 ? 0 : 1;  // HF sets the length-1 biases before it adds the others
        if (ra != rb) return ra < rb;
        return a.order < b.order;
    });
    std::vector<int32_t> h_ids, h_off{0}, h_ban, h_sid, h_soff;
    std::vector<float> h_bias;
    for (size_t q = 0; q < es.size(); ++q) {
        const Ent& e = es[q];
        if (q == 0 || es[q - 1].p[es[q - 1].len - 1] != e.p[e.len - 1]) {
            h_sid.push_back(e.p[e.len - 1]);
            h_soff.push_back((int32_t)q);
        }
        h_ids.insert(h_ids.end(), e.p, e.p + e.len);
        h_off.push_back((int32_t)h_ids.size());
        h_ban.push_back(e.ban);
        h_bias.push_back(e.bias);
    }
    h_soff.push_back((int32_t)es.size());
    auto t = std::make_shared<SeqTable>();
    (void)hipGetDevice(&t->device);  // (the callers have made the model's device current)
    t->n_seq = (int)es.size();
    t->n_slots = (int)h_sid.size();
    auto up = [](DevBuf& d, const void* src, size_t bytes) -> int {
        WMCHK(d.alloc(bytes));
        HIPCHK(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
        return 0;
    };
    WMCHK(up(t->ids, h_ids.data(), h_ids.size() * 4));
    WMCHK(up(t->off, h_off.data(), h_off.size() * 4));
    WMCHK(up(t->bias, h_bias.data(), h_bias.size() * 4));
    WMCHK(up(t->ban, h_ban.data(), h_ban.size() * 4));
    WMCHK(up(t->slot_id, h_sid.data(), h_sid.size() * 4));
    WMCHK(up(t->slot_off, h_soff.data(), h_soff.size() * 4));
    std::vector<int32_t> h_of((size_t)vocab, -1);
    for (size_t k = 0; k < h_sid.size(); ++k) h_of[h_sid[k]] = (int32_t)k;
    WMCHK(up(t->slot_of, h_of.data(), h_of.size() * 4));
    if (slot_ids) *slot_ids = h_sid;
    out = std::move(t);
    return 0;
}
extern "C" int wm_set_sequence_bias(wm_model* m, const int32_t* ids, const int32_t* offsets, const float* bias, int n_seq, const int32_t* bad_ids,
                                    const int32_t* bad_offsets, int n_bad) {
    if (!m) return fail(WM_E_ARG, "bad argument");
    HIPCHK(hipSetDevice(m->device));
    std::shared_ptr<SeqTable> t;
    WMCHK(build_seq_table(t, m->cfg.dims.vocab, ids, offsets, bias, n_seq, bad_ids, bad_offsets, n_bad));
    if (t) t->gen = ++m->seq_gen;
    m->repeat.sb = std::move(t);  // a held submit and a pending pass keep the table they were asked for with
    return 0;
}

// wm_transcribe_wait with the result left ON THE DEVICE as the gather buffer of the multi-GPU path: dev_packed
// [rows_cap, 1 + stride] int32 in the caller's device memory (e.g. a torch tensor), row r = [length, ids zero-padded]; rows past the
// batch are zeroed.  stride >= n_prompt + 1 + max_loop of the pass.
extern "C" int wm_transcribe_wait_device(wm_model* m, int slot, int32_t* dev_packed, int rows_cap, int stride) {
    if (!m || !dev_packed || slot < 0 || slot >= wm_model::NSLOT || stride <= 0) return fail(WM_E_ARG, "bad argument");
    PassOut out;
    out.dev_packed = dev_packed;
    out.rows_cap = rows_cap;
    out.pack_stride = stride;
    return collect_slot(m, slot, PassKind::transcribe, out);
}
extern "C" int wm_transcribe_steps(wm_model* m, int slot) {
    if (!m || slot < 0 || slot >= wm_model::NSLOT) return -1;
    return m->last_steps[slot];
}
