// kernels_frontend.hip — log-mel front end on the GPU: 16 kHz PCM -> [n_mels, n_frames] log-mel,
// the step immediately before the hot path.  The reference delegates it to HF's WhisperProcessor
// (export_weights.py:100-116).
//   frames_kernel      reflect-padded, Hann-windowed frames [rows, 416] fp32 (400 samples + 16 zero columns)
//   gemm_nt<float>     real DFT as an exact-fp32 MFMA GEMM against a [512, 416] cos / -sin basis (re at k, im at 256+k)
//   mel_log_kernel     |X|^2 -> sparse triangular mel filters -> log10(max(., 1e-10))
//   mel_norm_kernel    per-utterance max, clamp to max-8, (x+4)/4, channel-major output (what the encoder consumes)
// Long audio (wm_log_mel_long) runs the first three over chunks of frames at a frame offset t0 into a
// [B][n_mels][F] log-mel, then mel_max_partial_kernel + mel_norm_long_kernel: a two-stage per-utterance max over the whole
// spectrogram (no atomics) and a wide clamp / rescale pass.  window_gather_kernel cuts the encoder windows out of it.
// Chunked long-form: chunk_gather_kernel cuts overlapping chunks of PCM out of long recordings, one 30 s front-end row
// each, so that every chunk gets its own clamp max as HF's feature extractor gives it.
// Any sample rate and int16 in: resample_kernel<TIN> turns [B][stride_in] PCM at sr_in into fp32 PCM at 16 kHz by
// band-limited sinc interpolation (torchaudio.functional.resample's defaults), ahead of everything above.
#include "wm_kernels.h"

namespace wm {

__global__ __launch_bounds__(128) void frames_kernel(const float* __restrict__ pcm, float* __restrict__ F,
                                                     const float* __restrict__ window, int N, int n_frames, int hop, int t0) {
    const int t = blockIdx.x, b = blockIdx.y;
    const float* x = pcm + (size_t)b * N;
    float* row = F + ((size_t)b * n_frames + t) * 416;
    for (int n = threadIdx.x; n < 416; n += 128) {
        float v = 0.f;
        if (n < 400) {
            int i = hop * (t0 + t) + n - 200;
            if (i < 0) i = -i;                    // numpy 'reflect': edge sample not repeated
            if (i >= N) i = 2 * (N - 1) - i;
            v = x[i] * window[n];
        }
        row[n] = v;
    }
}
// x[b][i] = 0 for i >= len[b] (zero padding of short clips after the one-shot strided upload)
__global__ void zero_tails_kernel(float* __restrict__ pcm, const int* __restrict__ len, int N) {
    float* x = pcm + (size_t)blockIdx.y * N;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N && i >= len[blockIdx.y]) x[i] = 0.f;
}
void launch_zero_tails(float* pcm, const int* len, int B, int N, hipStream_t st) {
    hipLaunchKernelGGL(zero_tails_kernel, dim3((N + 255) / 256, B), dim3(256), 0, st, pcm, len, N);
}
void launch_frames(const float* pcm, float* F, const float* window, int B, int N, int n_frames, int hop, hipStream_t st, int t0) {
    hipLaunchKernelGGL(frames_kernel, dim3(n_frames, B), dim3(128), 0, st, pcm, F, window, N, n_frames, hop, t0);
}

// spec [rows][512] (re at k, im at 256+k) -> logmel[b][m][t].  One workgroup = 32 frames; power spectrum in LDS; thread
// (f, m-group) walks only the non-zero band [lo[m], hi[m]) of each triangular filter.
__global__ __launch_bounds__(256) void mel_log_kernel(const float* __restrict__ spec, const float* __restrict__ fb /*[201][n_mels]*/,
                                                      const int* __restrict__ band /*[n_mels][2]*/, float* __restrict__ logmel,
                                                      int n_frames, int n_mels, int out_frames, int t_out) {
    __shared__ float P[32][204];
    const int b = blockIdx.y, t0 = blockIdx.x * 32;
    for (int i = threadIdx.x; i < 32 * 201; i += 256) {
        const int f = i / 201, k = i % 201;
        float v = 0.f;
        if (t0 + f < n_frames) {
            const float* r = spec + ((size_t)b * n_frames + t0 + f) * 512;
            const float re = r[k], im = r[256 + k];
            v = re * re + im * im;
        }
        P[f][k] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 32 * n_mels; i += 256) {
        const int m = i / 32, f = i % 32;  // consecutive threads -> consecutive frames: coalesced stores along t
        if (t0 + f >= n_frames) continue;
        const int lo = band[2 * m], hi = band[2 * m + 1];
        float s = 0.f;
        for (int k = lo; k < hi; ++k) s += fb[k * n_mels + m] * P[f][k];
        logmel[((size_t)b * n_mels + m) * out_frames + t_out + t0 + f] = log10f(fmaxf(s, 1e-10f));
    }
}
// out_frames / t_out: row length of the output and frame offset of this chunk in it (0 / n_frames: one whole window)
void launch_mel_log(const float* spec, const float* fb, const int* band, float* logmel, int B, int n_frames, int n_mels, hipStream_t st,
                    int out_frames, int t_out) {
    hipLaunchKernelGGL(mel_log_kernel, dim3((n_frames + 31) / 32, B), dim3(256), 0, st, spec, fb, band, logmel, n_frames, n_mels,
                       out_frames > 0 ? out_frames : n_frames, t_out);
}

__global__ __launch_bounds__(1024) void mel_norm_kernel(const float* __restrict__ logmel, float* __restrict__ out, int n) {
    __shared__ float s_m[16];
    const float* x = logmel + (size_t)blockIdx.x * n;
    float* y = out + (size_t)blockIdx.x * n;
    float mx = -INFINITY;
    for (int i = threadIdx.x; i < n; i += 1024) mx = fmaxf(mx, x[i]);
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = s_m[0];
    for (int k = 1; k < 16; ++k) mx = fmaxf(mx, s_m[k]);
    const float floor_v = mx - 8.0f;
    for (int i = threadIdx.x; i < n; i += 1024) y[i] = (fmaxf(x[i], floor_v) + 4.0f) / 4.0f;
}
void launch_mel_norm(const float* logmel, float* out, int B, int n, hipStream_t st) {
    hipLaunchKernelGGL(mel_norm_kernel, dim3(B), dim3(1024), 0, st, logmel, out, n);
}

// Stage 1 of the long-audio max: block (p, b) reduces elements p·256 + i·P·256 + tid of utterance b's n values -> part[b][p].
// fmaxf is exact, so the result does not depend on the order; no atomics either way.
__global__ __launch_bounds__(256) void mel_max_partial_kernel(const float* __restrict__ x, float* __restrict__ part, size_t n) {
    __shared__ float s_m[4];
    const int P = gridDim.x;
    const float* xb = x + (size_t)blockIdx.y * n;
    float mx = -INFINITY;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)P * 256) mx = fmaxf(mx, xb[i]);
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) part[(size_t)blockIdx.y * P + blockIdx.x] = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]));
}
// Stage 2 + the wide pass: every block re-reduces utterance b's P partials (P <= 256, the same values in the same order in every
// block), then clamps / rescales its slice in place: y = (max(x, max - 8) + 4) / 4.
__global__ __launch_bounds__(256) void mel_norm_long_kernel(float* __restrict__ x, const float* __restrict__ part, int P, size_t n) {
    __shared__ float s_m[4];
    float mx = threadIdx.x < P ? part[(size_t)blockIdx.y * P + threadIdx.x] : -INFINITY;
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = mx;
    __syncthreads();
    const float floor_v = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3])) - 8.0f;
    float* xb = x + (size_t)blockIdx.y * n;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) xb[i] = (fmaxf(xb[i], floor_v) + 4.0f) / 4.0f;
}
void launch_mel_norm_long(float* logmel, float* part, int B, size_t n, hipStream_t st) {
    const int P = (int)std::min<size_t>(256, (n + 4095) / 4096);
    hipLaunchKernelGGL(mel_max_partial_kernel, dim3(P, B), dim3(256), 0, st, logmel, part, n);
    const int G = (int)std::min<size_t>(2048, (n + 1023) / 1024);
    hipLaunchKernelGGL(mel_norm_long_kernel, dim3(G, B), dim3(256), 0, st, logmel, part, P, n);
}

// Encoder windows of sequential long-form decoding: out[r][m][t] = mel[b][m][seek + t] for t < len, 0 beyond (HF's
// _get_input_segment pads with 0.0), for items[r] = (b, seek, len).  The host guarantees seek + len <= F.
__global__ __launch_bounds__(256) void window_gather_kernel(const float* __restrict__ mel, const int* __restrict__ items, float* __restrict__ out,
                                                            int n_mels, int F, int W) {
    const int t = blockIdx.x * 256 + threadIdx.x, m = blockIdx.y, r = blockIdx.z;
    if (t >= W) return;
    const int b = items[3 * r], seek = items[3 * r + 1], len = items[3 * r + 2];
    float v = 0.f;
    if (t < len && seek + t < F) v = mel[((size_t)b * n_mels + m) * F + seek + t];
    out[((size_t)r * n_mels + m) * W + t] = v;
}
void launch_window_gather(const float* mel, const int* items, float* out, int rows, int n_mels, int F, int W, hipStream_t st) {
    hipLaunchKernelGGL(window_gather_kernel, dim3((W + 255) / 256, n_mels, rows), dim3(256), 0, st, mel, items, out, n_mels, F, W);
}

// Chunks of chunked long-form transcription: out[r][i] = pcm[rec][start + i] for i < len, 0 beyond, for
// items[row0 + r] = (rec, start, len, ...) with `item_stride` ints per item.  pcm [R][T_max], out [rows][N].  The host guarantees
// start + len <= T_max and len <= N; the kernel clamps both again.  Offsets are formed in size_t: R · T_max passes 2^31 for an hour.
__global__ __launch_bounds__(256) void chunk_gather_kernel(const float* __restrict__ pcm, const int* __restrict__ items, int item_stride, int row0,
                                                           float* __restrict__ out, size_t T_max, int N) {
    const int r = blockIdx.y;
    const int* it = items + (size_t)(row0 + r) * item_stride;
    const size_t rec = (size_t)it[0], start = (size_t)it[1];
    const int len = min(it[2], N);
    const float* src = pcm + rec * T_max;
    float* dst = out + (size_t)r * N;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < N; i += gridDim.x * 256) dst[i] = (i < len && start + i < T_max) ? src[start + i] : 0.f;
}
void launch_chunk_gather(const float* pcm, const int* items, int item_stride, int row0, float* out, int rows, size_t T_max, int N, hipStream_t st) {
    const int gx = std::max(1, std::min(256, (N + 1023) / 1024));
    hipLaunchKernelGGL(chunk_gather_kernel, dim3(gx, rows), dim3(256), 0, st, pcm, items, item_stride, row0, out, T_max, N);
}

// Polyphase sinc resampler: y[j] = sum_k h[j % nw][k] * x[(j / nw) * orig - width + k], x zero outside [0, n_in[b]).
// One workgroup = `frames` input frames of one row = frames * nw consecutive outputs; the frames * orig + 2 * width input samples
// they read are staged in LDS once (every global read predicated on the row's length, int16 widened by an exact / 32768 on the way).
// The taps come compact and phase-minor from global memory: taps[q * nw + p] = h[p][lo[p] + q] for q < cnt[p], the non-zero span of
// phase p, so that the lanes of a wave (consecutive outputs = consecutive phases) read consecutive floats.  One fmaf chain per output
// in ascending k: a value depends on its own row's samples alone.  Sample indices are 64-bit: j * orig passes 2^31 within the hour.
template <typename TIN> __device__ inline float pcm_to_f32(TIN v);
template <> __device__ inline float pcm_to_f32<float>(float v) { return v; }
template <> __device__ inline float pcm_to_f32<int16_t>(int16_t v) { return (float)v * (1.0f / 32768.0f); }

template <typename TIN> __global__ __launch_bounds__(256) void resample_kernel(ResampleParams p) {
    extern __shared__ float s_x[];
    const int b = blockIdx.y;
    const int64_t n = p.n_in[b];
    const int64_t n_out = (n * p.nw + p.orig - 1) / p.orig;
    if (blockIdx.x == 0 && threadIdx.x == 0) p.n_out[b] = (int)n_out;
    const int64_t f0 = (int64_t)blockIdx.x * p.frames, j0 = f0 * p.nw;
    if (j0 >= n_out) return;  // the whole workgroup: no barrier is left behind
    const TIN* x = (const TIN*)p.x + (size_t)b * p.stride_in;
    const int64_t i0 = f0 * p.orig - p.width;
    const int span = p.frames * p.orig + 2 * p.width;
    for (int s = threadIdx.x; s < span; s += 256) {
        const int64_t i = i0 + s;
        s_x[s] = (i >= 0 && i < n) ? pcm_to_f32<TIN>(x[i]) : 0.f;
    }
    __syncthreads();
    float* y = p.y + (size_t)b * p.stride_out;
    const int outs = p.frames * p.nw;
    for (int jl = threadIdx.x; jl < outs; jl += 256) {
        const int64_t j = j0 + jl;
        if (j >= n_out) break;
        const int il = jl / p.nw, ph = jl - il * p.nw;
        const int lo = p.span[2 * ph], cnt = p.span[2 * ph + 1];  // lo + cnt <= 2 * width + orig: the reads stay inside the staged span
        const float* xs = s_x + il * p.orig + lo;
        const float* h = p.taps + ph;
        float acc = 0.f;
        for (int q = 0; q < cnt; ++q) acc = fmaf(h[(size_t)q * p.nw], xs[q], acc);
        y[j] = acc;
    }
}
int resample_frames(int orig, int nw, int width) {
    const int by_out = std::max(1, 1024 / nw), by_lds = (8192 - 2 * width) / orig;  // <= 1024 outputs and, where a frame allows, <= 32 KB
    return std::max(1, std::min(by_out, by_lds));
}
template <typename TIN> static int launch_resample_t(const ResampleParams& p, int B, int64_t max_n_out, hipStream_t st) {
    const size_t lds = ((size_t)p.frames * p.orig + 2 * (size_t)p.width) * 4;
    if (lds > 64 * 1024) return launch_refuse("resample: the input span of one frame does not fit in 64 KB of LDS");
    const int64_t per = (int64_t)p.frames * p.nw, gx = std::max<int64_t>(1, (max_n_out + per - 1) / per);
    if (gx > INT32_MAX || B > 65535) return launch_refuse("resample: more workgroups than a grid holds");
    if (lds > 48 * 1024)
        if (const hipError_t e = ensure_dyn_lds<&resample_kernel<TIN>>((int)lds); e != hipSuccess) return launch_hip_failed("resample LDS", e);
    hipLaunchKernelGGL((resample_kernel<TIN>), dim3((unsigned)gx, B), dim3(256), lds, st, p);
    return WM_LAUNCH_OK;
}
int launch_resample(const ResampleParams& p, bool in_i16, int B, int64_t max_n_out, hipStream_t st) {
    if (B <= 0 || p.orig <= 0 || p.nw <= 0 || p.width < 0 || p.frames <= 0 || max_n_out < 0) return launch_refuse("resample: bad shape");
    return in_i16 ? launch_resample_t<int16_t>(p, B, max_n_out, st) : launch_resample_t<float>(p, B, max_n_out, st);
}

}  // namespace wm
