// kernels_align.hip — token-level timestamps on gfx950: what HF WhisperGenerationMixin._extract_token_timestamps computes from the
// cross-attentions of the alignment heads, run after the greedy loop on the captured cross-q rows.
//
//   align_probs: s_rj = (0.125·q_r)·K_j over all n_audio_ctx keys, softmax over j            -> probs [B][n_sel][L][T]
//   align_norm : per column j < F_b: z = (w - mean_r) / std_r (population std, over the R_b rows), width-7 median along the columns
//                (reflect padding; skipped for F_b <= 3), mean over the heads                  -> M [B][L][T]
//   align_dtw  : DTW over -M (one workgroup per utterance, anti-diagonal sweep, 2-bit trace), backtrace, jump times -> times
//   align_window: a long-form window pass: the chain's ragged tables before it, the window's float64 times behind it
//
// Rows of an utterance: R_b = n_tokens[b] - n_prompt - 1 (the ids that were fed back; the last id has no row).  Nothing here reads
// anything the host computed after the loop: n_tokens stays on the device.  Forced alignment gives every utterance its
// own row count and output offset instead (AlignParams::rows / row0); the arithmetic is the same.
#include "wm_kernels.h"

#include <cmath>

namespace wm {

__device__ __forceinline__ int align_rows(const AlignParams& p, int b) {
    const int r = p.rows ? p.rows[b] : p.n_tokens[b] - p.n_prompt - 1;
    return r < 0 ? 0 : (r > p.L ? p.L : r);
}
__device__ __forceinline__ int align_cols(const AlignParams& p, int b) {
    if (!p.n_frames) return p.T;
    const int f = p.n_frames[b];
    return f < 1 ? 1 : (f > p.T ? p.T : f);
}
__device__ __forceinline__ float ld_f(const float* p, size_t i) { return p[i]; }
__device__ __forceinline__ float ld_f(const bf16* p, size_t i) { return (float)p[i]; }
__device__ __forceinline__ float ld_f(const f16* p, size_t i) { return (float)p[i]; }

// C[m][n] = scale · Σ_e A[m][e]·B[n][e] for one 64 x 64 tile, depth D (multiple of 32): 256 threads, 4 x 4 outputs each, fp32 FMA.
// Rows past m_valid / n_valid read zeros and are not stored.
template <typename TA, typename TB>
__device__ __forceinline__ void tile_nt(const TA* A, long lda, int m0, int m_valid, const TB* Bm, long ldb, int n0, int n_valid, int D,
                                        float scale, float* C, long ldc) {
    __shared__ float As[32][64 + 4];
    __shared__ float Bs[32][64 + 4];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    float acc[4][4] = {};
    for (int e0 = 0; e0 < D; e0 += 32) {
        // 64 rows x 32 depth of each operand: 8 elements per thread, consecutive threads along the depth (coalesced rows)
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int idx = tid + u * 256, row = idx >> 5, kk = idx & 31;
            const int ma = m0 + row, nb = n0 + row;
            As[kk][row] = ma < m_valid ? ld_f(A, (size_t)ma * lda + e0 + kk) : 0.f;
            Bs[kk][row] = nb < n_valid ? ld_f(Bm, (size_t)nb * ldb + e0 + kk) : 0.f;
        }
        __syncthreads();
#pragma unroll 8
        for (int kk = 0; kk < 32; ++kk) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(&As[kk][ty * 4]);
            const f32x4 bv = *reinterpret_cast<const f32x4*>(&Bs[kk][tx * 4]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] += a[i] * bv[j];
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + ty * 4 + i;
        if (m >= m_valid) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + tx * 4 + j;
            if (n < n_valid) C[(size_t)m * ldc + n] = acc[i][j] * scale;
        }
    }
}

// xattn path: K_h[b][k][j][c] = Σ_e X[b][j][e]·Wk[layer_k][head_k·64 + c][e] (the key projection the absorbed kernels never form;
// its bias is the same for every key and cancels in the softmax).  grid (ceil(T/64), n_sel, B)
__global__ __launch_bounds__(256) void align_kh_kernel(AlignParams p) {
    const int b = blockIdx.z, k = blockIdx.y;
    const bf16* X = (const bf16*)p.X + (size_t)b * p.T * p.d;
    const bf16* W = (const bf16*)p.Wk + ((size_t)(2 * p.layer[k]) * p.d + (size_t)p.head[k] * 64) * p.d;
    float* C = p.kh + ((size_t)b * p.n_sel + k) * p.T * 64;
    tile_nt<bf16, bf16>(X, p.d, blockIdx.x * 64, p.T, W, p.d, 0, 64, p.d, 1.f, C, 64);
}

// scores: probs[b][k][r][j] = (0.125·q)·K_j for r < R_b.  grid (ceil(T/64), ceil(L/64), B·n_sel)
template <typename TK> __global__ __launch_bounds__(256) void align_scores_kernel(AlignParams p) {
    const int b = blockIdx.z / p.n_sel, k = blockIdx.z % p.n_sel;
    const int R = align_rows(p, b), m0 = blockIdx.y * 64;
    if (m0 >= R) return;
    const float* Q = p.cap + (size_t)b * p.L * p.n_sel * 64 + (size_t)k * 64;
    const TK* K;
    long ldk;
    if (p.X) {
        K = (const TK*)(p.kh + ((size_t)b * p.n_sel + k) * p.T * 64);
        ldk = 64;
    } else {
        K = (const TK*)p.kv + (size_t)p.layer[k] * 2 * p.kv_layer_stride + (size_t)b * p.T * p.d + (size_t)p.head[k] * 64;
        ldk = p.d;
    }
    float* C = p.probs + ((size_t)b * p.n_sel + k) * p.L * p.T;
    // (0.125·q)·K = 0.125·(q·K) bit for bit: the scale is a power of two
    tile_nt<float, TK>(Q, (long)p.n_sel * 64, m0, R, K, ldk, blockIdx.x * 64, p.T, 64, 0.125f, C, p.T);
}

__device__ __forceinline__ float block_reduce(float v, bool is_max, float* red) {
    for (int o = 32; o > 0; o >>= 1) {
        const float u = __shfl_xor(v, o, 64);
        v = is_max ? fmaxf(v, u) : v + u;
    }
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    v = red[0];
    for (int i = 1; i < nw; ++i) v = is_max ? fmaxf(v, red[i]) : v + red[i];
    return v;
}

// softmax over all T keys of each row, in place.  grid (L, n_sel, B), 256 threads
__global__ __launch_bounds__(256) void align_softmax_kernel(AlignParams p) {
    const int b = blockIdx.z, k = blockIdx.y, r = blockIdx.x;
    if (r >= align_rows(p, b)) return;
    __shared__ float red[4];
    float* row = p.probs + (((size_t)b * p.n_sel + k) * p.L + r) * p.T;
    float mx = -INFINITY;
    for (int j = threadIdx.x; j < p.T; j += blockDim.x) mx = fmaxf(mx, row[j]);
    mx = block_reduce(mx, true, red);
    float sm = 0.f;
    for (int j = threadIdx.x; j < p.T; j += blockDim.x) sm += expf(row[j] - mx);
    sm = block_reduce(sm, false, red);
    for (int j = threadIdx.x; j < p.T; j += blockDim.x) row[j] = expf(row[j] - mx) / sm;
}

// column statistics over the R_b rows, float64 accumulation in row order: mean = Σw / R, std = sqrt(Σ(w - mean)² / R), both rounded
// to fp32 (the CPU restatement in tests/test_token_timestamps.py does exactly this).  grid (ceil(T/256), n_sel, B)
__global__ __launch_bounds__(256) void align_stats_kernel(AlignParams p) {
#pragma clang fp contract(off)
    const int b = blockIdx.z, k = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    const int R = align_rows(p, b);
    if (R == 0 || j >= align_cols(p, b)) return;
    const float* col = p.probs + ((size_t)b * p.n_sel + k) * p.L * p.T + j;
    double s = 0.0;
    for (int r = 0; r < R; ++r) s += (double)col[(size_t)r * p.T];
    const double mean = s / (double)R;
    double v = 0.0;
    for (int r = 0; r < R; ++r) {
        const double dv = (double)col[(size_t)r * p.T] - mean;
        const double sq = dv * dv;
        v += sq;
    }
    const size_t o = ((size_t)b * p.n_sel + k) * p.T + j;
    p.mean[o] = (float)mean;
    p.stdv[o] = (float)sqrt(v / (double)R);
}

// torch.sort order: NaN after every number
__device__ __forceinline__ void cswap(float& a, float& b) {
    const bool gt = isnan(a) ? !isnan(b) : (a > b);
    if (gt) {
        const float t = a;
        a = b;
        b = t;
    }
}
__device__ __forceinline__ float median7(float v[7]) {
    // optimal 16-comparator sorting network for 7 inputs; v[3] is the median
    cswap(v[0], v[6]); cswap(v[2], v[3]); cswap(v[4], v[5]);
    cswap(v[0], v[2]); cswap(v[1], v[4]); cswap(v[3], v[6]);
    cswap(v[0], v[1]); cswap(v[2], v[5]); cswap(v[3], v[4]);
    cswap(v[1], v[2]); cswap(v[4], v[6]);
    cswap(v[2], v[3]); cswap(v[4], v[5]);
    cswap(v[1], v[2]); cswap(v[3], v[4]); cswap(v[5], v[6]);
    return v[3];
}

// z-score, width-7 reflect median along the columns, mean over the heads (fp32, heads summed in order, then / n_sel).
// grid (ceil(T/256), L, B)
__global__ __launch_bounds__(256) void align_median_kernel(AlignParams p) {
#pragma clang fp contract(off)
    const int b = blockIdx.z, r = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    const int R = align_rows(p, b), F = align_cols(p, b);
    if (r >= R || j >= F) return;
    float acc = 0.f;
    for (int k = 0; k < p.n_sel; ++k) {
        const float* w = p.probs + (((size_t)b * p.n_sel + k) * p.L + r) * p.T;
        const float* mu = p.mean + ((size_t)b * p.n_sel + k) * p.T;
        const float* sd = p.stdv + ((size_t)b * p.n_sel + k) * p.T;
        float med;
        if (F <= 3) {
            med = (w[j] - mu[j]) / sd[j];
        } else {
            float v[7];
#pragma unroll
            for (int t = 0; t < 7; ++t) {
                int c = j + t - 3;
                c = c < 0 ? -c : (c >= F ? 2 * (F - 1) - c : c);  // reflect: the edge column is not repeated
                v[t] = (w[c] - mu[c]) / sd[c];
            }
            med = median7(v);
        }
        acc += med;
    }
    p.M[((size_t)b * p.L + r) * p.T + j] = acc / (float)p.n_sel;
}

// DTW over -M[b] (R_b x F_b), HF _dynamic_time_warping: fp32 cost, cost[i][j] = fp32(double(m) + double(c)) with c the diagonal c0
// only when strictly below both others, else c1 when strictly below both, else c2.  One workgroup per utterance, thread i owns row i
// (0..R), one barrier per anti-diagonal; the last three diagonals rotate through LDS.  The trace, 2 bits per cell, row-major in
// words of 16 columns: a thread's cells of one word are 16 consecutive diagonals, so it packs the word in a register and stores it
// once (no two threads share a word).  Then thread 0 walks back from (R, F); the last cell visited of text row i is where the
// forward path enters it: its column is the jump.
static __device__ __forceinline__ int trace_wpr(int T) { return (T + 15) >> 4; }

__global__ __launch_bounds__(512) void align_dtw_kernel(AlignParams p) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char dtw_smem[];
    const int b = blockIdx.x, i = threadIdx.x;
    const int R = align_rows(p, b), F = align_cols(p, b);
    const int L1 = p.L + 1, wpr = trace_wpr(p.T);
    float* diag = reinterpret_cast<float*>(dtw_smem);  // [3][L + 1]
    unsigned* tr = p.trace ? p.trace + (size_t)b * p.L * wpr : reinterpret_cast<unsigned*>(dtw_smem + (size_t)3 * L1 * 4);
    int* jt = reinterpret_cast<int*>(dtw_smem);  // after the sweep: jump column of each text row (reuses the diagonals)
    float* times = p.times + (size_t)b * p.out_stride;
    // ids [t_lo, n) carry a time; ragged rows: each utterance's own offset, and the id behind its last row is the last one
    const int t_lo = p.row0 ? p.row0[b] : p.n_prompt;
    const int n = p.rows ? t_lo + R + 1 : p.n_tokens[b];
    if (R > 0) {
        const float* Mrow = p.M + ((size_t)b * p.L + (i > 0 ? i - 1 : 0)) * p.T;
        const bool own = i >= 1 && i <= R;
        // diagonals 0 and 1: cost[0][0] = 0, every other boundary cell inf
        if (i <= R) {
            diag[0 * L1 + i] = i == 0 ? 0.f : INFINITY;
            diag[1 * L1 + i] = INFINITY;
        }
        __syncthreads();
        const int kend = R + F;
        // this thread's matrix entries of 16 diagonals at a time, the next 16 loaded one block ahead
        float cur[16], nxt[16];
        auto load16 = [&](int kb, float (&dst)[16]) {
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int j = kb + u - i;
                dst[u] = (own && j >= 1 && j <= F) ? Mrow[j - 1] : 0.f;
            }
        };
        load16(0, cur);
        unsigned word = 0;
        for (int kb = 0; kb <= kend; kb += 16) {
            load16(kb + 16, nxt);
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int k = kb + u;
                if (k >= 2 && k <= kend) {  // uniform over the workgroup
                    float* dc = diag + (k % 3) * L1;
                    const float* d1 = diag + ((k - 1) % 3) * L1;
                    const float* d2 = diag + ((k - 2) % 3) * L1;
                    if (i <= R) {
                        const int j = k - i;
                        float val = INFINITY;
                        if (i >= 1 && j >= 1 && j <= F) {
                            const float c0 = d2[i - 1], c1 = d1[i - 1], c2 = d1[i];
                            float c;
                            unsigned t;
                            if (c0 < c1 && c0 < c2) {
                                c = c0;
                                t = 0;
                            } else if (c1 < c0 && c1 < c2) {
                                c = c1;
                                t = 1;
                            } else {
                                c = c2;
                                t = 2;
                            }
                            val = (float)((double)(-cur[u]) + (double)c);
                            word |= t << (2 * ((j - 1) & 15));
                            if (((j - 1) & 15) == 15 || j == F) {
                                tr[(size_t)(i - 1) * wpr + ((j - 1) >> 4)] = word;
                                word = 0;
                            }
                        }
                        dc[i] = val;
                    }
                    __syncthreads();
                }
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) cur[u] = nxt[u];
        }
        __syncthreads();
        if (i == 0) {  // backtrace: trace[0][:] = 2, trace[:][0] = 1
            int ii = R, jj = F;
            while (ii > 0 || jj > 0) {
                if (ii > 0) jt[ii - 1] = jj - 1;
                unsigned t;
                if (ii == 0)
                    t = 2;
                else if (jj == 0)
                    t = 1;
                else
                    t = (tr[(size_t)(ii - 1) * wpr + ((jj - 1) >> 4)] >> (2 * ((jj - 1) & 15))) & 3u;
                if (t == 0) {
                    --ii;
                    --jj;
                } else if (t == 1) {
                    --ii;
                } else {
                    --jj;
                }
            }
        }
        __syncthreads();
    }
    // token times: 0 for the prompt, the R jump times (time index · 0.02 in double, stored fp32), the last id repeats the last one
    for (int t = i; t < p.out_stride; t += blockDim.x) {
        float v = 0.f;
        if (R > 0 && t >= t_lo && t < n) {
            const int r = t - t_lo < R ? t - t_lo : R - 1;
            v = (float)((double)jt[r] * 0.02);
        }
        times[t] = v;
    }
}

// A long-form window pass: mode 0 makes the chain's ragged tables from the counts the loop left on the device, mode 1
// turns the chain's [row][out_stride] times into each row's generated-id times at the window's offset.  The prompt length is clamped
// to [0, n_prompt] and the launcher requires out_stride >= n_prompt + L + 1, so no table value can move an access out of its row.
// grid (B), 256 threads
__global__ __launch_bounds__(256) void align_window_kernel(AlignWindowParams p) {
#pragma clang fp contract(off)
    const int r = blockIdx.x;
    int len = p.prompt_len ? p.prompt_len[r] : p.n_prompt;
    len = len < 0 ? 0 : (len > p.n_prompt ? p.n_prompt : len);
    int gen = p.n_tokens[r] - len;  // generated ids, the trailing eot included
    gen = gen < 0 ? 0 : (gen > p.L + 1 ? p.L + 1 : gen);
    if (p.mode == 0) {
        if (threadIdx.x == 0) {
            p.rows[r] = r < p.n_real && gen > 1 ? gen - 1 : 0;
            p.row0[r] = len;
        }
        return;
    }
    const bool real = r < p.n_real;  // (a row without align rows has zeros from the chain: its one id, if any, sits at the offset)
    const double off = (double)p.items[(size_t)r * 3 + 1] * 0.02 / 2;  // time_offset, as long_segments forms it
    const float* t = p.times + (size_t)r * p.out_stride + len;
    double* o = p.out + (size_t)r * (p.L + 1);
    for (int i = threadIdx.x; i <= p.L; i += blockDim.x) o[i] = real && i < gen ? (double)t[i] + off : 0.0;
}

int launch_align_window(const AlignWindowParams& p, hipStream_t st) {
    if (p.B <= 0 || p.n_real < 0 || p.n_real > p.B || p.L < 1 - p.mode || p.L > ALIGN_MAX_ROWS || p.n_prompt < 1 || p.out_stride < p.n_prompt + p.L + 1 ||
        (p.mode != 0 && p.mode != 1))
        return launch_refuse("align_window: bad shape");
    if (!p.n_tokens || !p.items || !p.rows || !p.row0 || (p.mode == 1 && (!p.times || !p.out))) return launch_refuse("align_window: null table");
    hipLaunchKernelGGL(align_window_kernel, dim3(p.B), dim3(256), 0, st, p);
    return WM_LAUNCH_OK;
}

int launch_align_probs(const AlignParams& p, hipStream_t st) {
    if (p.n_sel <= 0 || p.n_sel > ALIGN_MAX_HEADS || p.L <= 0 || p.L > ALIGN_MAX_ROWS || p.T <= 0 || p.d % 64)
        return launch_refuse("align_probs: bad shape");
    const dim3 blk(256);
    if (p.X) {
        if (p.d % 32) return launch_refuse("align_probs: d_model must be a multiple of 32");
        hipLaunchKernelGGL(align_kh_kernel, dim3((p.T + 63) / 64, p.n_sel, p.B), blk, 0, st, p);
        hipLaunchKernelGGL(align_scores_kernel<float>, dim3((p.T + 63) / 64, (p.L + 63) / 64, p.B * p.n_sel), blk, 0, st, p);
    } else if (p.kv_dtype == 0) {  // WM_F32
        hipLaunchKernelGGL(align_scores_kernel<float>, dim3((p.T + 63) / 64, (p.L + 63) / 64, p.B * p.n_sel), blk, 0, st, p);
    } else if (p.kv_dtype == 1) {  // WM_BF16
        hipLaunchKernelGGL(align_scores_kernel<bf16>, dim3((p.T + 63) / 64, (p.L + 63) / 64, p.B * p.n_sel), blk, 0, st, p);
    } else {
        hipLaunchKernelGGL(align_scores_kernel<f16>, dim3((p.T + 63) / 64, (p.L + 63) / 64, p.B * p.n_sel), blk, 0, st, p);
    }
    hipLaunchKernelGGL(align_softmax_kernel, dim3(p.L, p.n_sel, p.B), blk, 0, st, p);
    return WM_LAUNCH_OK;
}

int launch_align_norm(const AlignParams& p, hipStream_t st) {
    if (p.n_sel <= 0 || p.n_sel > ALIGN_MAX_HEADS || p.L <= 0 || p.L > ALIGN_MAX_ROWS || p.T <= 0) return launch_refuse("align_norm: bad shape");
    hipLaunchKernelGGL(align_stats_kernel, dim3((p.T + 255) / 256, p.n_sel, p.B), dim3(256), 0, st, p);
    hipLaunchKernelGGL(align_median_kernel, dim3((p.T + 255) / 256, p.L, p.B), dim3(256), 0, st, p);
    return WM_LAUNCH_OK;
}

static const size_t ALIGN_LDS_MAX = 150 * 1024;  // gfx950: 160 KiB of LDS per workgroup
size_t align_dtw_lds_bytes(int L, int T) {
    const size_t b = (size_t)3 * (L + 1) * 4 + (size_t)L * ((T + 15) / 16) * 4;
    return b <= ALIGN_LDS_MAX ? b : 0;
}

int launch_align_dtw(const AlignParams& p, hipStream_t st) {
    if (!p.rows != !p.row0) return launch_refuse("align_dtw: rows and row0 go together");
    if (p.L <= 0 || p.L > ALIGN_MAX_ROWS || p.T <= 0 || p.out_stride < (p.rows ? p.out_need : p.n_prompt + p.L + 1))
        return launch_refuse("align_dtw: bad shape");
    size_t lds = p.trace ? (size_t)3 * (p.L + 1) * 4 : align_dtw_lds_bytes(p.L, p.T);
    if (lds == 0) return launch_refuse("align_dtw: the trace does not fit in LDS and no global trace buffer was given");
    const hipError_t e = ensure_dyn_lds<align_dtw_kernel>((int)lds);
    if (e != hipSuccess) return launch_hip_failed("align_dtw LDS attribute", e);
    const int threads = (p.L + 1 + 63) / 64 * 64;
    hipLaunchKernelGGL(align_dtw_kernel, dim3(p.B), dim3(threads), lds, st, p);
    return WM_LAUNCH_OK;
}

}  // namespace wm
