// kernels_decoder.hip — the HBM-bound half of the path: one KV-cached decode step for B utterances.
//
// Replaces (reference file:line): the M<=4 branch of matmul (whisper_tensor.mojo:158-175) for every decoder
// projection incl. the tied 51 865-way logits (whisper.mojo:162-166); layer_norm (whisper_tensor.mojo:249-285) fused
// as a prologue; gelu (:288-308) and the residual adds (layers.mojo:457-461,483-487,513-517) fused as epilogues;
// the KV-cache append (layers.mojo:140-147); the q_len==1 attention path (layers.mojo:186-272); the embedding +
// position add (whisper.mojo:141-149); argmax (whisper_tensor.mojo:431-439).
#include "wm_kernels.h"

#include <cstdio>
#include <cstdlib>
#include <type_traits>

namespace wm {

// ------------------------------------------------------------------------------------------------------------
// Developer timeline: ts[0] = entry count, then (tag, 100 MHz clock) pairs; tag = owner id << 8 | kind
// (0 cross-attention start, 1 merge start, 2 logits start, 3 argmax start).  Off (null) outside WM_TRACE_EVENTS=<file>.
__device__ __forceinline__ void ts_put(long long* ts, int id, int kind) {
    const unsigned long long i = atomicAdd((unsigned long long*)ts, 1ull);
    if (i < (1ull << 20)) {
        ts[1 + 2 * i] = ((long long)id << 8) | kind;
        ts[2 + 2 * i] = (long long)wall_clock64();
    }
}

// x[b] = token_emb[tok[b]] + pos_emb[pos[b]]      (whisper.mojo:141-149)
__global__ void dec_embed_kernel(const float* __restrict__ tok_emb, const float* __restrict__ pos_emb,
                                 const int* __restrict__ tok, const int* __restrict__ pos, float* __restrict__ x, int d) {
    const int b = blockIdx.x;
    const float* t = tok_emb + (size_t)tok[b] * d;
    const float* p = pos_emb + (size_t)pos[b] * d;
    for (int j = threadIdx.x; j < d; j += blockDim.x) x[(size_t)b * d + j] = t[j] + p[j];
}
void launch_dec_embed(const float* tok_emb, const float* pos_emb, const int* tok, const int* pos, float* x, int B, int d,
                      hipStream_t st) {
    hipLaunchKernelGGL(dec_embed_kernel, dim3(B), dim3(128), 0, st, tok_emb, pos_emb, tok, pos, x, d);
}

// ------------------------------------------------------------------------------------------------------------
// Skinny linear: out[B,N] = epi( pro(x)[B,K] · W[N,K]ᵀ + bias ).  Every weight byte is read from HBM once per step,
// all B rows sharing the pass — the batched form of the reference's "parallel over n, dot over K" GEMV
// (whisper_tensor.mojo:158-175).
//
// These launches move 0.3-1.2 MB: they are LATENCY bound, and what they wait for is (a) one memory round trip and
// (b) the serial instruction stream of a wave (a lone wave retires ~1 instruction per 4-5 cycles: 1 700 instructions
// = 4 us, measured).  So the kernel minimises the per-wave stream:
//   * workgroup = one 16x16 output tile (16 utterances x 16 columns); its NW <= 16 waves split K, wave w owning
//     k-steps w, w+NW, … (KPW = 1 for K = d_model): a wave's whole job is KPW weight fragments, KPW activation
//     fragments and KPW MFMAs, everything requested up front;
//   * LayerNorm prologue: row statistics (one-pass variance, as the reference) from the SAME activation registers —
//     8·KPW values per lane, a 4-lane butterfly, one LDS exchange between the NW waves;
//   * computed as outᵀ (A-operand = weight fragment): a lane owns 4 consecutive columns of one utterance; the NW
//     K-partials meet in LDS and wave 0 finishes (bias / GELU / residual / KV-cache append), with its epilogue operands
//     requested before anything else so they ride the same round trip.
// dtype-tagged store of one fp32 value / four fp32 values (out_dtype: 0 fp32, 1 bf16, 2 f16)
__device__ __forceinline__ void store_as(void* base, size_t idx, float v, int dt) {
    if (dt == 0)
        ((float*)base)[idx] = v;
    else if (dt == 1)
        ((bf16*)base)[idx] = (bf16)v;
    else
        ((f16*)base)[idx] = (f16)v;
}

// KG > 1 (K = 3072, fc2 of d_model 768: 96 k-steps = 16 waves x KG = 2 groups x KPW = 3; K = 4096, fc2 of d_model 1024: 2 x 4): a wave walks KG groups of KPW k-steps, k-step
// w + NW·(kg·KPW + i), into the same accumulators; one LDS exchange at the end, as ever.  The loop is NOT unrolled: group kg + 1's
// fragments reuse group kg's registers (fp32, two column tiles: 48 + 24 fragment VGPRs instead of 96 + 48 — 144 do not fit the 128 a
// 1024-thread workgroup leaves a wave), at the price of one memory round trip per group.  KG = 1 is the kernel as it always was.
template <typename TW, int KPW, bool LN, int NT, bool XT = false, int KG = 1>
__global__ __launch_bounds__(1024) void dec_linear_kernel(DecLinearParams p) {
    static_assert(!(LN && XT), "the LayerNorm prologue reads the fp32 residual stream");
    static_assert(!(LN && KG > 1), "the LayerNorm statistics need the whole row before the first MFMA");
#ifdef WM_DEV
#define WM_DL_STAMP(k) do { if (p.dbg && (threadIdx.x & 63) == 0) p.dbg[(((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 16 + (threadIdx.x >> 6)) * 8 + (k)] = (long long)wall_clock64(); } while (0)
#else
#define WM_DL_STAMP(k) do { } while (0)
#endif
    WM_DL_STAMP(0);
    // dynamic LDS, sized by the launcher for the NW waves actually used: [NW][NT][64] f32x4 K-partials, then [NW][16][2]
    // LayerNorm statistics (24.6 + 1.5 KB for the 12-wave QKV / fc1 launches: fits beside two 64-KB GEMM workgroups)
    extern __shared__ __attribute__((aligned(16))) unsigned char dl_smem[];
    f32x4 (*s_red)[NT][64] = reinterpret_cast<f32x4 (*)[NT][64]>(dl_smem);
    float (*s_stat)[16][2] = reinterpret_cast<float (*)[16][2]>(dl_smem + (size_t)(blockDim.x >> 6) * NT * 64 * sizeof(f32x4));
    // LayerNorm gamma | beta of each wave's k-steps, [NW][KPW][32 gamma, 32 beta]: ONE 4-byte load per lane and k-step, handed to
    // the 16 lanes that need each value through LDS.  (Every lane fetching its own 8 + 8 values was four 1-KB load instructions per
    // k-step — 40 % of what an LN1+QKV workgroup put through its CU's address path: 64 B per clock is what bounds these launches.)
    float (*s_gbl)[KPW][64] = reinterpret_cast<float (*)[KPW][64]>(dl_smem + (size_t)(blockDim.x >> 6) * (NT * 64 * sizeof(f32x4) + 16 * 2 * sizeof(float)));
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * (16 * NT), b0 = blockIdx.y * 16;
    int xrow = b0 + r16;
    xrow = xrow < p.B ? xrow : p.B - 1;
    const TW* wp[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        int wrow = n0 + t * 16 + r16;
        wrow = wrow < p.N ? wrow : p.N - 1;
        wp[t] = (const TW*)p.W + (size_t)wrow * p.K + g * 8;
    }
    const float* xp = p.x + (size_t)xrow * p.ldx + g * 8;
    const TW* xpt = (const TW*)p.x + (size_t)xrow * p.ldx + g * 8;  // XT: the same row in operand dtype
    // epilogue operands (wave t finishes column tile t)
    const int eb = b0 + r16, en = n0 + (w < NT ? w : 0) * 16 + g * 4;
    // a second column tile that starts past the (16-padded) width does not exist: storing it would land in the next row
    const bool epi = w < NT && eb < p.B && n0 + (w < NT ? w : 0) * 16 < ((p.N + 15) & ~15);
    float bias4[4] = {0.f, 0.f, 0.f, 0.f};
    f32x4 res4 = f32x4{0.f, 0.f, 0.f, 0.f};
    int cache_row = 0;
    if (epi) {
        if (p.bias) {
#pragma unroll
            for (int r = 0; r < 4; ++r) bias4[r] = p.bias[min(en + r, p.N - 1)];
        }
        if (p.residual) res4 = *reinterpret_cast<const f32x4*>(p.residual + (size_t)eb * p.ldr + en);
        // (the address is uniform, so hipcc emits a scalar load whatever the source says — kernarg -> ctl -> len is one more
        //  scalar round trip in the prologue; in-kernel stamps showed the prologue's scalar stages are not what delays the loads)
        if (p.kcache) cache_row = __builtin_nontemporal_load(&p.ctl->len);
        if (p.cap && !p.cap_map) cache_row = __builtin_nontemporal_load(&p.ctl->len);
    }
    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int kg = 0; kg < KG; ++kg) {
    Frag<TW> wf[NT][KPW];
    Frag<TW> xft[XT ? KPW : 1];
    f32x4 xa[XT ? 1 : KPW][2];
    float gbv[LN ? KPW : 1];
    // every weight load first: they come from HBM / MALL (~1 us), the activation and LayerNorm loads behind them are L2 hits,
    // and a wave issues loads only as fast as the CU's address path takes them (24 x 1 KB per wave here)
#pragma unroll
    for (int i = 0; i < KPW; ++i) {
        const int k = (w + nw * (kg * KPW + i)) * 32;
#pragma unroll
        for (int t = 0; t < NT; ++t) wf[t][i] = load_frag<TW>(wp[t] + k);
    }
#pragma unroll
    for (int i = 0; i < KPW; ++i) {
        const int k = (w + nw * (kg * KPW + i)) * 32;
        if constexpr (XT) {
            xft[i] = load_frag<TW>(xpt + k);
        } else {
            xa[i][0] = *reinterpret_cast<const f32x4*>(xp + k);
            xa[i][1] = *reinterpret_cast<const f32x4*>(xp + k + 4);
        }
        if (LN) gbv[i] = (lane < 32 ? p.ln_g : p.ln_b - 32)[k + lane];
    }
    WM_DL_STAMP(1);
    float mean = 0.f, rstd = 1.f;
    if constexpr (LN) {
        float sm = 0.f, sq = 0.f;
#pragma unroll
        for (int i = 0; i < KPW; ++i)
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float v = xa[i][h2][j];
                    sm += v;
                    sq += v * v;
                }
        sm += __shfl_xor(sm, 16, 64);
        sq += __shfl_xor(sq, 16, 64);
        sm += __shfl_xor(sm, 32, 64);
        sq += __shfl_xor(sq, 32, 64);
        if (g == 0) {
            s_stat[w][r16][0] = sm;
            s_stat[w][r16][1] = sq;
        }
#pragma unroll
        for (int i = 0; i < KPW; ++i) s_gbl[w][i][lane] = gbv[i];
        __syncthreads();
        sm = 0.f;
        sq = 0.f;
        for (int k = 0; k < nw; ++k) {
            sm += s_stat[k][r16][0];
            sq += s_stat[k][r16][1];
        }
        mean = sm / (float)p.K;
        const float var = (sq / (float)p.K) - (mean * mean);
        rstd = 1.0f / sqrtf(fmaxf(var, 0.f) + 1e-5f);
    }
    WM_DL_STAMP(2);
#pragma unroll
    for (int i = 0; i < KPW; ++i) {
        Frag<TW> xf;
        if constexpr (XT) {
            xf = xft[i];
        } else {
            float xv[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                xv[j] = xa[i][0][j];
                xv[4 + j] = xa[i][1][j];
            }
            if (LN) {
                const f32x4 gm0 = *reinterpret_cast<const f32x4*>(&s_gbl[w][i][g * 8]), gm1 = *reinterpret_cast<const f32x4*>(&s_gbl[w][i][g * 8 + 4]);
                const f32x4 bt0 = *reinterpret_cast<const f32x4*>(&s_gbl[w][i][32 + g * 8]), bt1 = *reinterpret_cast<const f32x4*>(&s_gbl[w][i][32 + g * 8 + 4]);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    xv[j] = (xv[j] - mean) * rstd * gm0[j] + bt0[j];
                    xv[4 + j] = (xv[4 + j] - mean) * rstd * gm1[j] + bt1[j];
                }
            }
            xf = make_frag<TW>(xv);
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = mma32(wf[t][i], xf, acc[t]);
    }
    }  // kg
#pragma unroll
    for (int t = 0; t < NT; ++t) s_red[w][t][lane] = acc[t];
    WM_DL_STAMP(3);
    __syncthreads();
    WM_DL_STAMP(4);
    if (epi) {
        f32x4 v = s_red[0][w][lane];
        for (int k = 1; k < nw; ++k) v += s_red[k][w][lane];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += bias4[r];
        if (p.act) {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = gelu_f(v[r], p.gelu_mode);
        }
        v += res4;
        if (p.kcache && en >= p.d_model) {
            const bool is_v = en >= 2 * p.d_model;
            const int cc = en - (is_v ? 2 : 1) * p.d_model;
            const int ub = p.kv_B > 0 ? eb % p.kv_B : eb, ut = p.kv_B > 0 ? eb / p.kv_B : 0;  // prefill rows: (position, utterance)
            const size_t off = (size_t)ub * p.kv_batch_stride + (size_t)(cache_row + ut) * p.d_model + cc;
            void* basep = is_v ? p.vcache : p.kcache;
            if (p.kv_dtype == 0) {
                *reinterpret_cast<f32x4*>((float*)basep + off) = v;
            } else if (p.kv_dtype == 1) {
                bf16x4 o = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
                *reinterpret_cast<bf16x4*>((bf16*)basep + off) = o;
            } else {
                f16x4 o = {(f16)v[0], (f16)v[1], (f16)v[2], (f16)v[3]};
                *reinterpret_cast<f16x4*>((f16*)basep + off) = o;
            }
        } else if (p.out_is_t && sizeof(TW) == 2) {
            typedef __attribute__((ext_vector_type(4))) TW t4;
            const t4 o = {from_f32<TW>(v[0]), from_f32<TW>(v[1]), from_f32<TW>(v[2]), from_f32<TW>(v[3])};
            *reinterpret_cast<t4*>((TW*)p.out + (size_t)eb * p.ldo + en) = o;
        } else {
            *reinterpret_cast<f32x4*>(p.out + (size_t)eb * p.ldo + en) = v;
        }
        if (p.cap) {  // alignment-head capture: this lane's 4 columns lie in one head
            const int h = en >> 6, step = cache_row - p.cap_step0;
            const int k = h < 32 ? p.cap_sel[h] : -1;
            if (p.cap_map) {  // by row map: the position-major rows of a teacher-forced pass go to their utterance's row
                // (the empty asm pins the map's address arithmetic to this branch: hoisted to the prologue it cost every instantiation
                //  with one column tile two VGPRs, and two of them a wave of occupancy)
                int idx = eb;
                asm volatile("" : "+v"(idx));
                const int dr = k >= 0 ? p.cap_map[idx] : -1;
                if (dr >= 0) *reinterpret_cast<f32x4*>(p.cap + ((size_t)dr * p.cap_nsel + k) * 64 + (en & 63)) = v;
            } else if (k >= 0 && step >= 0 && step < p.cap_steps)
                *reinterpret_cast<f32x4*>(p.cap + (size_t)eb * p.cap_row_stride + ((size_t)step * p.cap_nsel + k) * 64 + (en & 63)) = v;
        }
    }
    WM_DL_STAMP(5);
}
#undef WM_DL_STAMP
// K past 2048, the K-long form: 16 waves walking KG groups of KPW k-steps.  K = 3072 (fc2 of d_model 768) is 2 groups of 3, K = 4096
// (fc2 of d_model 1024, 128 k-steps) 2 groups of 4: fp32 with two column tiles holds wf[2][4] + xa[4][2] = 64 + 32 fragment VGPRs of
// the 128 a 1024-thread workgroup leaves a wave, and 4 groups of 2 would pay two more memory round trips for registers nobody needs.
// No LayerNorm form: a row of 3072 / 4096 columns is an MLP hidden row, never the residual stream.
static const int DEC_LINEAR_K_LONG = 3072, DEC_LINEAR_K_LONG2 = 4096;
template <typename TW, int KPW, int KG> static int launch_dec_linear_long_t(const DecLinearParams& p, hipStream_t st) {
    constexpr int NW = 16;
    if (p.K != NW * KPW * KG * 32) return launch_refuse("dec_linear: the k-step groups do not cover K");
    const bool wide = p.N >= 1024;
    const dim3 grid((p.N + (wide ? 31 : 15)) / (wide ? 32 : 16), (p.B + 15) / 16), block(NW * 64);
    const size_t smem = (size_t)NW * (wide ? 2 : 1) * 64 * sizeof(f32x4) + (size_t)NW * 16 * 2 * sizeof(float);
    if (sizeof(TW) == 2 && p.x_is_t) {
        if (wide)
            hipLaunchKernelGGL((dec_linear_kernel<TW, KPW, false, 2, true, KG>), grid, block, smem, st, p);
        else
            hipLaunchKernelGGL((dec_linear_kernel<TW, KPW, false, 1, true, KG>), grid, block, smem, st, p);
    } else {
        if (wide)
            hipLaunchKernelGGL((dec_linear_kernel<TW, KPW, false, 2, false, KG>), grid, block, smem, st, p);
        else
            hipLaunchKernelGGL((dec_linear_kernel<TW, KPW, false, 1, false, KG>), grid, block, smem, st, p);
    }
    return WM_LAUNCH_OK;
}
template <typename TW> static int launch_dec_linear_long(const DecLinearParams& p, hipStream_t st) {
    if (p.ln_g) return launch_refuse("dec_linear: no LayerNorm prologue at K = 3072 / 4096");
    if (p.K == DEC_LINEAR_K_LONG2) return launch_dec_linear_long_t<TW, 4, 2>(p, st);
    return launch_dec_linear_long_t<TW, 3, 2>(p, st);
}
template <typename TW, int KPW> static int launch_dec_linear_t(const DecLinearParams& p, int nw, hipStream_t st) {
    // two column tiles per workgroup for the wide projections (QKV, fc1): half the workgroups, one activation
    // fragment (and one LayerNorm) feeding two MFMAs
    static const int nt_force = wm_env("WM_LIN_NT") ? atoi(wm_env("WM_LIN_NT")) : 0;  // dev A/B
    const bool wide = nt_force ? nt_force == 2 : (p.N >= 1024 && nw >= 2);
    const dim3 grid((p.N + (wide ? 31 : 15)) / (wide ? 32 : 16), (p.B + 15) / 16), block(nw * 64);
    auto smem = [&](int nt) {  // K-partials, LayerNorm statistics, LayerNorm gamma | beta (see the kernel)
        return (size_t)nw * nt * 64 * sizeof(f32x4) + (size_t)nw * 16 * 2 * sizeof(float) + (p.ln_g ? (size_t)nw * KPW * 64 * sizeof(float) : 0);
    };
    if (p.ln_g) {
        if (wide)
            hipLaunchKernelGGL((dec_linear_kernel<TW, KPW, true, 2>), grid, block, smem(2), st, p);
        else
            hipLaunchKernelGGL((dec_linear_kernel<TW, KPW, true, 1>), grid, block, smem(1), st, p);
    } else if (sizeof(TW) == 2 && p.x_is_t) {  // activations already in operand dtype (attention output, MLP hidden)
        if (wide)
            hipLaunchKernelGGL((dec_linear_kernel<TW, KPW, false, 2, true>), grid, block, smem(2), st, p);
        else
            hipLaunchKernelGGL((dec_linear_kernel<TW, KPW, false, 1, true>), grid, block, smem(1), st, p);
    } else {
        if (wide)
            hipLaunchKernelGGL((dec_linear_kernel<TW, KPW, false, 2>), grid, block, smem(2), st, p);
        else
            hipLaunchKernelGGL((dec_linear_kernel<TW, KPW, false, 1>), grid, block, smem(1), st, p);
    }
    return WM_LAUNCH_OK;
}
// K % 32 == 0 and (K/32) must factor as NW * KPW with NW <= 16, KPW <= 4 (true for every K = 128·j, j <= 16).
static int dec_linear_waves(int K, int elem_bytes = 2) {
    if (K <= 0 || (K & 31)) return 0;
    const int ksteps = K >> 5;
    if (elem_bytes == 4) {  // fp32 operands (eight exact-fp32 MFMAs per k-step): one k-step per wave stays fastest (B = 1: 211 vs 223 us per step)
        static const int kpw32 = wm_env("WM_LIN_KPW32") ? atoi(wm_env("WM_LIN_KPW32")) : 0;  // dev A/B: k-steps per wave for fp32 operands
        if (kpw32 > 0) {
            for (int lim = kpw32; lim <= 4; ++lim)
                for (int c = 1; c <= 16; ++c)
                    if (ksteps % c == 0 && ksteps / c <= lim) return c;
        }
        for (int c = 16; c >= 1; --c)
            if (ksteps % c == 0 && ksteps / c <= 4) return c;
        return 0;
    }
    // the FEWEST waves whose k-steps-per-wave stay <= 3 (else <= 4): measured on MI355X (round 2, tiny B = 64) 4 waves x 3 k-steps
    // for K = 384 beat 12 waves x 1 (decode step 266 -> 257 us; pass alone 33.3 -> 32.4 ms) — a 256-thread workgroup is
    // dispatched sooner, exchanges 4 instead of 12 partials, and fits beside a K/V-streaming kernel of another pass; 6 x 2
    // (263 us), 3 x 4 (274 us) and 2 x 6 (363 us) lost
    static const int kpw_max = wm_env("WM_LIN_KPW") ? atoi(wm_env("WM_LIN_KPW")) : 3;
    for (int lim = kpw_max; lim <= 4; ++lim)
        for (int c = 1; c <= 16; ++c)
            if (ksteps % c == 0 && ksteps / c <= lim) return c;
    return 0;
}
bool dec_linear_supports_k(int K) { return dec_linear_waves(K) > 0 || K == DEC_LINEAR_K_LONG; }
// what a model's ffn and wm_op_dec_linear_long may be: the above and K = 4096.  (wm_op_dec_linear and wm_op_matmul_nt keep the
// narrower answer: their refusal of K = 4096 is part of their contract.)
bool dec_linear_long_supports_k(int K) { return K == DEC_LINEAR_K_LONG || K == DEC_LINEAR_K_LONG2; }
bool dec_linear_model_supports_k(int K) { return dec_linear_supports_k(K) || K == DEC_LINEAR_K_LONG2; }
template <typename TW> int launch_dec_linear(const DecLinearParams& p, hipStream_t st) {
    if (p.B <= 0 || p.N <= 0) return launch_refuse("dec_linear: empty problem");
    if (dec_linear_long_supports_k(p.K)) return launch_dec_linear_long<TW>(p, st);
    const int ksteps = p.K >> 5;
    const int nw = dec_linear_waves(p.K, (int)sizeof(TW));
    if (nw == 0)  // refuse rather than drop k-steps (check_cfg / wm_op_matmul_nt keep model paths away from here)
        return launch_refuse("dec_linear: K must be a multiple of 32 whose k-steps split over <= 16 waves x <= 4 steps (K <= 2048), or 3072 / 4096");
    switch (ksteps / nw) {
        case 1: return launch_dec_linear_t<TW, 1>(p, nw, st);
        case 2: return launch_dec_linear_t<TW, 2>(p, nw, st);
        case 3: return launch_dec_linear_t<TW, 3>(p, nw, st);
        default: return launch_dec_linear_t<TW, 4>(p, nw, st);
    }
}
template int launch_dec_linear<float>(const DecLinearParams&, hipStream_t);
template int launch_dec_linear<bf16>(const DecLinearParams&, hipStream_t);
template int launch_dec_linear<f16>(const DecLinearParams&, hipStream_t);

// Scratch of the logits epilogue (fused argmax, stage 1): static LDS in the 16-bit kernel; in the split-fp32 kernel it overlays the
// activation images once every wave is past its last fragment read.
template <int NRB> struct LogitsScratch {
    float (*av)[NRB * 16];  // [8 waves x 4 lane groups][utterance row]: the 4 lane groups of a row meet in LDS, not by cross-lane
    int (*ai)[NRB * 16];    // shuffles (two ds_bpermute round trips per row block on the kernel's tail)
    float (*tv)[NRB * 16];  // [8 waves][row]: timestamp-side partials (best value, max, sum of exp)
    float (*tm)[NRB * 16];
    float (*ts)[NRB * 16];
    int (*ti)[NRB * 16];
    float (*ls)[NRB * 16];  // [8 waves][row], log-prob kernels only: sum of exp(v - wave max) over the wave's admissible text candidates
    static constexpr size_t bytes = (size_t)(2 * 32 + 4 * 8) * NRB * 16 * 4;
    static constexpr size_t bytes_lp = bytes + (size_t)8 * NRB * 16 * 4;
    __device__ static LogitsScratch carve(unsigned char* base) {
        LogitsScratch s;
        float* f = reinterpret_cast<float*>(base);
        s.av = reinterpret_cast<float (*)[NRB * 16]>(f);
        s.ai = reinterpret_cast<int (*)[NRB * 16]>(f + 32 * NRB * 16);
        s.tv = reinterpret_cast<float (*)[NRB * 16]>(f + 64 * NRB * 16);
        s.tm = reinterpret_cast<float (*)[NRB * 16]>(f + 72 * NRB * 16);
        s.ts = reinterpret_cast<float (*)[NRB * 16]>(f + 80 * NRB * 16);
        s.ti = reinterpret_cast<int (*)[NRB * 16]>(f + 88 * NRB * 16);
        s.ls = reinterpret_cast<float (*)[NRB * 16]>(f + 96 * NRB * 16);  // past `bytes`: touched by the log-prob kernels only
        return s;
    }
};
// Shared tail of the logits kernels.  acc[nb][rb][r] = logits[row0 + 16 rb + r16][n0[nb] + 4 g + r]: optional store of the
// logits, then the fused argmax's stage 1 (and the timestamp-side partials when the rules are on).
// LP (log-probabilities): also the text side of the softmax normaliser — per part the sum of exp(v - amax_val) over the
// candidates the argmax admits (same mask, same [text_lo, text_hi) test), amax_val being their maximum: every term is <= 1, so a
// logits row offset by 1e4 cannot overflow.  LP = false compiles to exactly the kernel without it.
template <int NRB, bool LP>
__device__ __forceinline__ void logits_epilogue(const DecLinearParams& p, int CT, const f32x4 (&acc)[2][NRB], const int (&n0)[2],
                                                const bool (&have)[2], const float (&mk)[2][4], int row0, int nrows, int lane, int w,
                                                const LogitsScratch<NRB>& sc) {
    const int r16 = lane & 15, g = lane >> 4;
    // acc[nb][rb][r] = logits[row0 + 16 rb + r16][n0[nb] + 4 g + r]
    if (p.out) {
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb) {
            const int lr = rb * 16 + r16;
            if (lr < nrows) {
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
                    const int n = n0[nb] + g * 4;
                    if (have[nb] && n < p.ldo) *reinterpret_cast<f32x4*>(p.out + (size_t)(row0 + lr) * p.ldo + n) = acc[nb][rb];
                }
            }
        }
    }
    if (p.amax_val) {
        // fused argmax, stage 1 (whisper_tensor.mojo:431-439: lowest index wins): this workgroup's best of its CT*16
        // columns per utterance.  Lane-local over 8 columns, 2 butterfly steps over the 4 lanes of a row, LDS over waves.
        // Timestamp rules on (p.ts_state): "best" is the best admissible TEXT id of the utterance's range, and the workgroups
        // that cover timestamp ids also reduce the admissible timestamps to (best value, its id, max, sum of exp(v - max)) —
        // what stage 2 needs to compare the timestamps' probability mass with the best text id (HF rule 5).
        const bool ts_on = p.ts_state != nullptr;
        const bool wg_ts = ts_on && (int)((blockIdx.x + 1) * CT * 16) > p.ts_begin;  // workgroup-uniform
        float (*s_av)[NRB * 16] = sc.av;
        int (*s_ai)[NRB * 16] = sc.ai;
        float (*s_tv)[NRB * 16] = sc.tv, (*s_tm)[NRB * 16] = sc.tm, (*s_ts)[NRB * 16] = sc.ts;
        int (*s_ti)[NRB * 16] = sc.ti;
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb) {
            float bv = -INFINITY;
            int bi = 0x7fffffff;
            int t_lo = 0, t_hi = 0x7fffffff, q_lo = 0, q_hi = 0;
            if (ts_on) {
                const TsState* stp = p.ts_state + row0 + min(rb * 16 + r16, nrows - 1);
                t_lo = stp->text_lo;
                t_hi = stp->text_hi;
                q_lo = stp->ts_lo;
                q_hi = stp->ts_hi;
            }
            float cand[2][4];
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int n = n0[nb] + g * 4 + r;
                    const float v = acc[nb][rb][r] + mk[nb][r];  // 0 or -inf
                    cand[nb][r] = v;
                    if (have[nb] && n < p.N && n >= t_lo && n < t_hi && v > bv) {  // n increases through the loop: strict '>' keeps the lowest index
                        bv = v;
                        bi = n;
                    }
                }
            if constexpr (LP) {
                float ls = 0.f, lm = bv;  // the lane's maximum IS its best value
#pragma unroll
                for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int n = n0[nb] + g * 4 + r;
                        if (have[nb] && n < p.N && n >= t_lo && n < t_hi && cand[nb][r] > -INFINITY) ls += expf(cand[nb][r] - lm);
                    }
#pragma unroll
                for (int o = 16; o <= 32; o <<= 1) {  // the 4 lanes of a row (lane group 0 holds the value that is kept)
                    const float m2 = __shfl_xor(lm, o, 64), s2 = __shfl_xor(ls, o, 64);
                    const float mn = fmaxf(lm, m2);
                    ls = (ls > 0.f ? ls * expf(lm - mn) : 0.f) + (s2 > 0.f ? s2 * expf(m2 - mn) : 0.f);
                    lm = mn;
                }
                if (g == 0) sc.ls[w][rb * 16 + r16] = ls;  // relative to the wave's maximum = max of its four s_av entries
            }
            if (wg_ts) {
                float tv = -INFINITY, tsum = 0.f;
                int ti = 0x7fffffff;
#pragma unroll
                for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int n = n0[nb] + g * 4 + r;
                        if (have[nb] && n < p.N && n >= q_lo && n < q_hi && cand[nb][r] > tv) {
                            tv = cand[nb][r];
                            ti = n;
                        }
                    }
                float tm = tv;  // the lane's max IS its best value
#pragma unroll
                for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int n = n0[nb] + g * 4 + r;
                        if (have[nb] && n < p.N && n >= q_lo && n < q_hi && cand[nb][r] > -INFINITY) tsum += expf(cand[nb][r] - tm);
                    }
#pragma unroll
                for (int o = 16; o <= 32; o <<= 1) {
                    const float v2 = __shfl_xor(tv, o, 64), m2 = __shfl_xor(tm, o, 64), s2 = __shfl_xor(tsum, o, 64);
                    const int i2 = __shfl_xor(ti, o, 64);
                    if (v2 > tv || (v2 == tv && i2 < ti)) {
                        tv = v2;
                        ti = i2;
                    }
                    const float mn = fmaxf(tm, m2);
                    tsum = (tsum > 0.f ? tsum * expf(tm - mn) : 0.f) + (s2 > 0.f ? s2 * expf(m2 - mn) : 0.f);
                    tm = mn;
                }
                if (g == 0) {
                    s_tv[w][rb * 16 + r16] = tv;
                    s_ti[w][rb * 16 + r16] = ti;
                    s_tm[w][rb * 16 + r16] = tm;
                    s_ts[w][rb * 16 + r16] = tsum;
                }
            }
            s_av[w * 4 + g][rb * 16 + r16] = bv;
            s_ai[w * 4 + g][rb * 16 + r16] = bi;
        }
        __syncthreads();
        if (threadIdx.x < NRB * 16 && (int)threadIdx.x < nrows) {
            float bv = s_av[0][threadIdx.x];
            int bi = s_ai[0][threadIdx.x];
#pragma unroll
            for (int k = 1; k < 8 * 4; ++k) {
                const float v2 = s_av[k][threadIdx.x];
                const int i2 = s_ai[k][threadIdx.x];
                if (v2 > bv || (v2 == bv && i2 < bi)) {
                    bv = v2;
                    bi = i2;
                }
            }
            const size_t o = (size_t)(row0 + threadIdx.x) * p.amax_stride + blockIdx.x;
            p.amax_val[o] = bv;
            p.amax_idx[o] = bi;
            if constexpr (LP) {  // the 8 waves' sums in wave order, rescaled to the part's maximum bv
                float tot = 0.f;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const float wm = fmaxf(fmaxf(s_av[4 * k][threadIdx.x], s_av[4 * k + 1][threadIdx.x]),
                                           fmaxf(s_av[4 * k + 2][threadIdx.x], s_av[4 * k + 3][threadIdx.x]));
                    const float s2 = sc.ls[k][threadIdx.x];
                    if (s2 > 0.f) tot += s2 * expf(wm - bv);
                }
                p.lp_s[o] = tot;
            }
            if (wg_ts) {  // the 8 waves' timestamp partials, in wave order (deterministic)
                float tv = s_tv[0][threadIdx.x], tm = s_tm[0][threadIdx.x], tsum = s_ts[0][threadIdx.x];
                int ti = s_ti[0][threadIdx.x];
#pragma unroll
                for (int k = 1; k < 8; ++k) {
                    const float v2 = s_tv[k][threadIdx.x], m2 = s_tm[k][threadIdx.x], s2 = s_ts[k][threadIdx.x];
                    const int i2 = s_ti[k][threadIdx.x];
                    if (v2 > tv || (v2 == tv && i2 < ti)) {
                        tv = v2;
                        ti = i2;
                    }
                    const float mn = fmaxf(tm, m2);
                    tsum = (tsum > 0.f ? tsum * expf(tm - mn) : 0.f) + (s2 > 0.f ? s2 * expf(m2 - mn) : 0.f);
                    tm = mn;
                }
                p.ts_val[o] = tv;
                p.ts_idx[o] = ti;
                p.ts_m[o] = tm;
                p.ts_s[o] = tsum;
            }
        }
    }
}
// RP (repetition processors): the lane's accumulators pass through the row's two bit sets first — penalty at the ids of
// `seen`, -inf at the ids of `ban` — and the tail above sees the processed values: the logits store, the argmax candidates, the
// timestamp partials and the log-prob sums.  A lane's four columns start at a multiple of four, so one word of each set covers them.
// RP = false is the tail above and nothing else.
// SB (sequence bias / bad words; needs RP): a third word per column group, the row's `hit` bits.  Where one is set the
// table's id -> slot map names the row's SeqSlot: its summed bias is added BEFORE the penalty, and a ban makes the value -inf at once
// — bit for bit what HF's later `+ -inf` leaves, since the penalty (p > 0) and the n-gram ban keep -inf, and it frees the flag's
// register across the rest (the 128-row fp32 kernel has none to spare).
template <int NRB, bool LP, bool RP, bool SB = false>
__device__ __forceinline__ void logits_epilogue_rp(const DecLinearParams& p, int CT, const f32x4 (&acc)[2][NRB], const int (&n0)[2],
                                                   const bool (&have)[2], const float (&mk)[2][4], int row0, int nrows, int lane, int w,
                                                   const LogitsScratch<NRB>& sc) {
    static_assert(RP || !SB, "the sequence bias rides the repetition processors' instantiation");
    if constexpr (RP) {
        const int r16 = lane & 15, g = lane >> 4;
        const float pen = p.rp_ctl->penalty;
        const int* slot_of = nullptr;  // SB: the table's id -> slot map, one uniform load for the whole epilogue
        if constexpr (SB) slot_of = p.sb_ctl->slot_of;
        f32x4 pa[2][NRB];
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb) {
            const size_t urow = (size_t)(row0 + min(rb * 16 + r16, nrows - 1));
            const size_t row = urow * p.rp_words;
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                const int n = min(n0[nb] + g * 4, p.N - 1);  // (a tile past the vocabulary is not `have`: any word of the row will do)
                const unsigned sw = p.rp_seen[row + (n >> 5)] >> (n & 31), bw = p.rp_ban[row + (n >> 5)] >> (n & 31);
                unsigned hw = 0u;
                if constexpr (SB) hw = (p.sb_hit[row + (n >> 5)] >> (n & 31)) & 15u;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float z = acc[nb][rb][r];
                    if constexpr (SB) {
                        if ((hw >> r) & 1u) {  // (a set bit is an id below N that has a slot)
                            const SeqSlot e = p.sb_val[urow * SEQ_BIAS_MAX + slot_of[n + r]];
                            z = (e.flags & 2) ? -INFINITY : z + e.bias;
                        }
                    }
                    if ((sw >> r) & 1u) z = z < 0.f ? z * pen : z / pen;
                    if ((bw >> r) & 1u) z = -INFINITY;
                    pa[nb][rb][r] = z;
                }
            }
        }
        logits_epilogue<NRB, LP>(p, CT, pa, n0, have, mk, row0, nrows, lane, w, sc);
    } else {
        logits_epilogue<NRB, LP>(p, CT, acc, n0, have, mk, row0, nrows, lane, w, sc);
    }
}

// ------------------------------------------------------------------------------------------------------------
// Final LayerNorm + tied-embedding logits (whisper.mojo:156-166): logits[B, V] = LN(x)[B, d] · tok_emb[V, d]ᵀ.
// 80 MB (fp32) / 40 MB (16-bit) of weights per step: the one decoder GEMM that is bandwidth- rather than
// latency-bound.  Workgroup = 128 vocabulary rows x up to 64 utterances: the normalised activations are built ONCE per
// workgroup (LN statistics from a 4-thread-per-row sweep, everything in flight at once) and parked in LDS as MFMA
// operands, so L2 sees x once per 128 columns; each wave then streams its 32 embedding rows straight from HBM into
// registers (all k-steps in flight) and needs no cross-wave reduction.
template <typename TW, int KD /* d_model/128 */, int NRB, bool LP = false, bool RP = false, bool SB = false>
__global__ __launch_bounds__(512) void dec_logits_kernel(DecLinearParams p, int CT) {
    // One workgroup = 8 waves = CT <= 16 column tiles of 16 vocabulary rows (wave w owns tiles w and w+8), all NRB*16
    // utterance rows.  CT is chosen by the launcher so that the whole vocabulary is ONE round of <= 256 workgroups
    // (51 865 rows: CT = 13 -> 250 workgroups, 160 KB of embedding rows per CU): the kernel is a single pass over the
    // embedding at one workgroup per CU instead of 406 128-column workgroups in two rounds (16.5 -> ~10 us).
    constexpr int K = KD * 128;
    // row pitch of the LDS activation image: for 16-bit operands ≡ 40 dwords (mod 64) — with the hardware's ds_read_b128
    // lane groups ({0-3,12-15,20-27}, ...) the 16 fragment rows of one read then sit on disjoint banks (a 4-dword pad
    // left one 2-way conflict per group: 3 % of the kernel's wave cycles in SQ_LDS_BANK_CONFLICT)
    constexpr int PAD = sizeof(TW) == 2 ? 80 - (K % 128) : 16 / sizeof(TW);
    constexpr int PITCH = K + PAD;
    constexpr int KS = KD * 4;                         // k-steps of 32
    // k-steps whose weight fragments are in flight together: every panel of a tile for 16-bit operands and half of them for fp32 up to
    // d_model 512 (128 fragment VGPRs for the two tiles); at d_model 768 (24 k-steps) half of that again — 96 VGPRs, not 192 — rather
    // than spill.  Chunk c > 0 is loaded at the head of chunk c into the registers chunk c - 1 just multiplied from: there is no
    // explicit prefetch here (the split kernel below has one), any overlap is the scheduler's and the other wave's of the SIMD
    // At d_model 1024 (32 k-steps) a quarter: 8 k-steps for 16-bit, 4 for fp32 — 64 VGPRs for the two tiles (a third, 10.67, is no whole
    // chunk, and a half would be 128 VGPRs, past the 96 that d_model 768 holds)
    constexpr int CHK = (sizeof(TW) == 2 ? KS : KS / 2) / (KD > 6 ? 4 : KD > 4 ? 2 : 1);
    static_assert(KS % CHK == 0, "whole chunks");
    static_assert(2 * K <= 4 * 512, "gamma | beta are fetched as one float4 per thread");
#ifndef WM_LOGITS_PRE
#define WM_LOGITS_PRE 4
#endif
    constexpr int PRE = WM_LOGITS_PRE < CHK ? WM_LOGITS_PRE : CHK;  // k-steps of the first tile requested before the staging arithmetic
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    TW* xs = reinterpret_cast<TW*>(smem_raw);  // [NRB*16][PITCH]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int row0 = blockIdx.y * NRB * 16;
    if (p.ts && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) ts_put(p.ts, p.ts_id, 2);
#ifdef WM_DEV
#define WM_LG_STAMP(k) do { if (p.dbg && (threadIdx.x & 63) == 0) p.dbg[((size_t)blockIdx.x * 8 + (threadIdx.x >> 6)) * 8 + (k)] = (long long)wall_clock64(); } while (0)
#else
#define WM_LG_STAMP(k) do { } while (0)
#endif
    WM_LG_STAMP(0);
    const int nrows = min(NRB * 16, p.B - row0);
    int n0[2];
    bool have[2];
    const TW* wp[2];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const int t = w + 8 * nb;  // column tile inside this workgroup
        n0[nb] = (blockIdx.x * CT + t) * 16;
        have[nb] = __builtin_amdgcn_readfirstlane((int)(t < CT && n0[nb] < p.N)) != 0;  // wave-uniform, and the compiler knows
        int wr = n0[nb] + r16;
        wr = wr < p.N ? wr : p.N - 1;
        wp[nb] = (const TW*)p.W + (size_t)wr * K + g * 8;
    }
    // a wave without a second tile re-requests its first one (same lines: L1 / L2 hits, no extra HBM traffic) so that the loads
    // below are UNCONDITIONAL: with a branch around them hipcc's s_waitcnt bookkeeping can no longer count them and makes the
    // LayerNorm staging wait for every embedding row (vmcnt(11) … vmcnt(0) in front of the statistics: 5 us of the kernel)
    if (!have[1]) wp[1] = wp[0];
    // The activation rows are requested first; the embedding rows once they are here (see below), so the LayerNorm staging
    // runs while this wave's embedding rows stream from HBM.
    Frag<TW> wf[2][CHK];
    float mk[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};  // additive argmax mask (0 / -inf) of this lane's columns
    __shared__ __attribute__((aligned(16))) float s_gb[2][K];  // LN gamma / beta, fetched ahead of the embedding rows too
    {  // LN + convert -> LDS.  thread t: row t>>3 (+64 per pass), eighth t&7 of the row, float4 index q + 8*i
        for (int rbase = 0; rbase < NRB * 16; rbase += 64) {
            const int lr = rbase + (threadIdx.x >> 3), q = threadIdx.x & 7;
            f32x4 v[KD * 4];
            const bool mine = lr < NRB * 16;
            if (mine) {
                const int row = min(lr, nrows - 1);
                const float* xr = p.x + (size_t)(row0 + row) * p.ldx;
#pragma unroll
                for (int i = 0; i < KD * 4; ++i) v[i] = *reinterpret_cast<const f32x4*>(xr + 4 * (q + 8 * i));
            }
            if (rbase == 0) {
                f32x4 gbv = f32x4{0.f, 0.f, 0.f, 0.f};
                const int gi = threadIdx.x;  // float4 index into [gamma | beta]
                if (gi < K / 2) gbv = *reinterpret_cast<const f32x4*>((gi < K / 4 ? p.ln_g : p.ln_b - K) + 4 * gi);
                if (p.amax_mask) {  // the argmax mask of this lane's 8 columns rides the same round trip (the epilogue used to fetch it)
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                        for (int r = 0; r < 4; ++r) mk[nb][r] = p.amax_mask[min(n0[nb] + g * 4 + r, p.N - 1)];
                }
                if (gi < K / 2) *reinterpret_cast<f32x4*>(&s_gb[0][0] + 4 * gi) = gbv;
                WM_LG_STAMP(5);
                __syncthreads();
                WM_LG_STAMP(6);
                // The embedding rows are requested only now, when this workgroup's activation rows have arrived: issued together
                // with them (round 1) the 40 MB burst of all 250 workgroups filled the memory pipeline first and the 98 KB of
                // activations every workgroup needs — the same L2 lines for all of them — came back last: the LayerNorm staging
                // ended 7.8 us after kernel entry, 1.7 us before the MFMAs did (in-kernel stamps, tools/logits_phases.py).
#pragma unroll
                for (int i = 0; i < PRE; ++i) wf[0][i] = load_frag<TW>(wp[0] + i * 32);
            }
            if (mine) {
                float sm = 0.f, sq = 0.f;
#pragma unroll
                for (int i = 0; i < KD * 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        sm += v[i][j];
                        sq += v[i][j] * v[i][j];
                    }
#pragma unroll
                for (int o = 1; o <= 4; o <<= 1) {
                    sm += __shfl_xor(sm, o, 64);
                    sq += __shfl_xor(sq, o, 64);
                }
                const float mean = sm / (float)K;
                const float var = (sq / (float)K) - (mean * mean);
                const float rstd = 1.0f / sqrtf(fmaxf(var, 0.f) + 1e-5f);
#pragma unroll
                for (int i = 0; i < KD * 4; ++i) {
                    const int k = 4 * (q + 8 * i);
                    const f32x4 gm = *reinterpret_cast<const f32x4*>(&s_gb[0][k]), bt = *reinterpret_cast<const f32x4*>(&s_gb[1][k]);
                    typedef __attribute__((ext_vector_type(4))) TW t4;
                    t4 o;
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[j] = from_f32<TW>((v[i][j] - mean) * rstd * gm[j] + bt[j]);
                    *reinterpret_cast<t4*>(&xs[lr * PITCH + k]) = o;
                }
            }
        }
    }
    WM_LG_STAMP(1);
    __syncthreads();
    WM_LG_STAMP(2);
    // the rest of the embedding rows, behind the staging arithmetic AND the barrier: a wave cannot issue past a vector load the
    // memory pipeline has no room for, so with all 24 KB per wave requested up front the staging stood behind the loads' ISSUE
    // for ~5 us (in-kernel stamps), and a barrier after the issue made every wave wait for the slowest issuer
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int i = (nb == 0 ? PRE : 0); i < CHK; ++i) wf[nb][i] = load_frag<TW>(wp[nb] + i * 32);

    f32x4 acc[2][NRB];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb) acc[nb][rb] = f32x4{0.f, 0.f, 0.f, 0.f};
    // straight-line MFMA bodies for "both tiles" / "first tile only" (have[1] implies have[0]); a per-MFMA predicate
    // would put a branch and a wait around every instruction
    auto body = [&](auto NB) {
        constexpr int nbn = decltype(NB)::value;
#pragma unroll
        for (int c = 0; c < KS / CHK; ++c) {
            if (c > 0) {
#pragma unroll
                for (int nb = 0; nb < nbn; ++nb)
#pragma unroll
                    for (int i = 0; i < CHK; ++i) wf[nb][i] = load_frag<TW>(wp[nb] + (c * CHK + i) * 32);
            }
#pragma unroll
            for (int i = 0; i < CHK; ++i) {
#pragma unroll
                for (int rb = 0; rb < NRB; ++rb) {
                    Frag<TW> xf = load_frag<TW>(&xs[(rb * 16 + r16) * PITCH + (c * CHK + i) * 32 + g * 8]);
#pragma unroll
                    for (int nb = 0; nb < nbn; ++nb) acc[nb][rb] = mma32(wf[nb][i], xf, acc[nb][rb]);
                }
            }
        }
    };
    if (have[1])
        body(std::integral_constant<int, 2>{});
    else if (have[0])
        body(std::integral_constant<int, 1>{});
    WM_LG_STAMP(3);
    if constexpr (NRB <= 4) {
        __shared__ float s_av[8 * 4][NRB * 16];
        __shared__ int s_ai[8 * 4][NRB * 16];
        __shared__ float s_tv[8][NRB * 16], s_tm[8][NRB * 16], s_ts[8][NRB * 16];
        __shared__ int s_ti[8][NRB * 16];
        LogitsScratch<NRB> sc;
        sc.av = s_av;
        sc.ai = s_ai;
        sc.tv = s_tv;
        sc.tm = s_tm;
        sc.ts = s_ts;
        sc.ti = s_ti;
        sc.ls = nullptr;
        if constexpr (LP) {
            __shared__ float s_ls[8][NRB * 16];
            sc.ls = s_ls;
        }
        logits_epilogue_rp<NRB, LP, RP, SB>(p, CT, acc, n0, have, mk, row0, nrows, lane, w, sc);
    } else {  // 128 rows: the 48 KB of scratch do not fit beside the activation image — overlay it once every wave is done reading
        __syncthreads();
        static_assert((LP ? LogitsScratch<NRB>::bytes_lp : LogitsScratch<NRB>::bytes) <= (size_t)NRB * 16 * PITCH * sizeof(TW),
                      "epilogue scratch must fit the activation image");
        logits_epilogue_rp<NRB, LP, RP, SB>(p, CT, acc, n0, have, mk, row0, nrows, lane, w, LogitsScratch<NRB>::carve(smem_raw));
    }
    WM_LG_STAMP(4);
}
#undef WM_LG_STAMP
int dec_logits_tiles_per_wg(int N);
int dec_logits_parts(int N);
// ------------------------------------------------------------------------------------------------------------
// The same projection for FP32 weights (decoder_fp32 / all-fp32 models) on the bf16 MFMA pipe.
// With fp32 operands the kernel above is MFMA-bound, not HBM-bound: 2·64·51 865·384 = 2.55 GFLOP per step against the 157 TFLOP/s
// of v_mfma_f32_16x16x4_f32 (32 cycles per SIMD for a 16x16x4 block) is 16 us at best, 20.5 us for the busiest SIMD's four
// column tiles — measured 38 us per launch for an 80 MB stream that HBM delivers in 13.  gfx950 has no reduced-precision fp32
// path, but every fp32 value is EXACTLY the sum of three bf16 values (8 + 8 + 8 significant bits, taken by truncation:
// x = h + m + l with l = x - h - m exact), and a bf16 x bf16 product is exact in the MFMA's fp32 accumulator.  So
//     w·x = (wh + wm + wl)(xh + xm + xl) ≈ wh·xh + wh·xm + wm·xh + wh·xl + wm·xm + wl·xh
// — six v_mfma_f32_16x16x32_bf16 (16 cycles each, K = 32) instead of eight fp32 MFMAs of K = 4 (32 cycles each): 96 against 256
// cycles per 16x16x32 block.  The three dropped terms (wm·xl, wl·xm, wl·xl) are < 2^-21 |w·x| together in the worst case
// (truncation leaves |m| < 2^-7 |x|, |l| < 2^-15 |x|), 2^-24 typically; accumulation stays fp32.  Measured over 5 clips x 196
// positions x 51 865 logits: largest deviation from the fp32 CPU restatement 5.3e-6, against 6.3e-6 for the exact-fp32 MFMA kernel (tests/test_split3.py
// restates the arithmetic; tests/test_gpu_long_parity.py prints the figure).  The weights are split in registers as they arrive (44 VALU operations per fragment, hidden in
// the MFMAs' issue gaps); the normalised activations are split ONCE per workgroup and parked in LDS as three bf16 images.
struct Split3 {
    bf16x8 h, m, l;
};
__device__ __forceinline__ Split3 split3(const f32x8& x) {
    typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;
    u16x8 h, m, l;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const unsigned u = __float_as_uint(x[j]);
        const unsigned uh = u & 0xffff0000u;  // top 8 significant bits (truncation keeps the sign: the remainders share it)
        const float r1 = x[j] - __uint_as_float(uh);  // exact
        const unsigned um = __float_as_uint(r1) & 0xffff0000u;
        const float r2 = r1 - __uint_as_float(um);  // exact, <= 8 significant bits left: a bf16 value
        h[j] = (unsigned short)(uh >> 16);
        m[j] = (unsigned short)(um >> 16);
        l[j] = (unsigned short)(__float_as_uint(r2) >> 16);
    }
    Split3 s;
    s.h = __builtin_bit_cast(bf16x8, h);
    s.m = __builtin_bit_cast(bf16x8, m);
    s.l = __builtin_bit_cast(bf16x8, l);
    return s;
}
__device__ __forceinline__ f32x4 mma_bf16(const bf16x8& a, const bf16x8& b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

template <int KD /* d_model/128 */, int NRB, bool LP = false, bool RP = false, bool SB = false>
__global__ __launch_bounds__(512) void dec_logits_split_kernel(DecLinearParams p, int CT) {
    // Geometry as dec_logits_kernel: 8 waves, wave w owns column tiles w and w + 8 of the workgroup's CT <= 16, all NRB*16 rows.
    constexpr int K = KD * 128;
    // row pitch of one bf16 activation image: ≡ 8 dwords (mod 64) — the 16 fragment rows of a ds_read_b128 lane group
    // ({rows 0-3, 12-15 at k-group g} ∪ {rows 4-11 at g + 1}) then sit on 16 disjoint 4-bank groups, like the ≡ 40 pitch above
    constexpr int PITCH = K + 16;
    constexpr int KS = KD * 4;      // k-steps of 32
    constexpr int CHK = KD == 1 ? 2 : KS / 2;  // k-steps of a tile whose fp32 weight fragments are in flight together (8 VGPRs each)
    constexpr int IMG = NRB * 16 * PITCH;  // elements per image
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    bf16* xs = reinterpret_cast<bf16*>(smem_raw);                                        // [3][NRB*16][PITCH]: h, m, l
    float* s_gb = reinterpret_cast<float*>(smem_raw + (size_t)3 * IMG * sizeof(bf16));  // [2][K] LN gamma / beta
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int row0 = blockIdx.y * NRB * 16;
    if (p.ts && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) ts_put(p.ts, p.ts_id, 2);
#ifdef WM_DEV
#define WM_LG_STAMP(k) do { if (p.dbg && (threadIdx.x & 63) == 0) p.dbg[((size_t)blockIdx.x * 8 + (threadIdx.x >> 6)) * 8 + (k)] = (long long)wall_clock64(); } while (0)
#else
#define WM_LG_STAMP(k) do { } while (0)
#endif
    WM_LG_STAMP(0);
    const int nrows = min(NRB * 16, p.B - row0);
    int n0[2];
    bool have[2];
    const float* wp[2];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const int t = w + 8 * nb;
        n0[nb] = (blockIdx.x * CT + t) * 16;
        have[nb] = __builtin_amdgcn_readfirstlane((int)(t < CT && n0[nb] < p.N)) != 0;
        int wr = n0[nb] + r16;
        wr = wr < p.N ? wr : p.N - 1;
        wp[nb] = (const float*)p.W + (size_t)wr * K + g * 8;
    }
    if (!have[1]) wp[1] = wp[0];  // unconditional loads (see dec_logits_kernel): a wave without a second tile re-requests its first
    f32x8 wf[2][CHK];
    auto wload = [&](int nb, int ks) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(wp[nb] + ks * 32), b = *reinterpret_cast<const f32x4*>(wp[nb] + ks * 32 + 4);
        return f32x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    };
    float mk[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    constexpr int PRE = CHK < 4 ? CHK : 4;  // k-steps of the first tile requested before the staging arithmetic
    {  // LN + three-way split -> LDS.  thread t: row t>>3 (+64 per pass), eighth t&7 of the row, float4 index q + 8*i
        for (int rbase = 0; rbase < NRB * 16; rbase += 64) {
            const int lr = rbase + (threadIdx.x >> 3), q = threadIdx.x & 7;
            f32x4 v[KD * 4];
            const bool mine = lr < NRB * 16;
            if (mine) {
                const int row = min(lr, nrows - 1);
                const float* xr = p.x + (size_t)(row0 + row) * p.ldx;
#pragma unroll
                for (int i = 0; i < KD * 4; ++i) v[i] = *reinterpret_cast<const f32x4*>(xr + 4 * (q + 8 * i));
            }
            if (rbase == 0) {
                f32x4 gbv = f32x4{0.f, 0.f, 0.f, 0.f};
                const int gi = threadIdx.x;  // float4 index into [gamma | beta]
                if (gi < K / 2) gbv = *reinterpret_cast<const f32x4*>((gi < K / 4 ? p.ln_g : p.ln_b - K) + 4 * gi);
                if (p.amax_mask) {
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                        for (int r = 0; r < 4; ++r) mk[nb][r] = p.amax_mask[min(n0[nb] + g * 4 + r, p.N - 1)];
                }
                if (gi < K / 2) *reinterpret_cast<f32x4*>(s_gb + 4 * gi) = gbv;
                WM_LG_STAMP(5);
                __syncthreads();
                WM_LG_STAMP(6);
#pragma unroll
                for (int i = 0; i < PRE; ++i) wf[0][i] = wload(0, i);
            }
            if (mine) {
                float sm = 0.f, sq = 0.f;
#pragma unroll
                for (int i = 0; i < KD * 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        sm += v[i][j];
                        sq += v[i][j] * v[i][j];
                    }
#pragma unroll
                for (int o = 1; o <= 4; o <<= 1) {
                    sm += __shfl_xor(sm, o, 64);
                    sq += __shfl_xor(sq, o, 64);
                }
                const float mean = sm / (float)K;
                const float var = (sq / (float)K) - (mean * mean);
                const float rstd = 1.0f / sqrtf(fmaxf(var, 0.f) + 1e-5f);
#pragma unroll
                for (int i = 0; i < KD * 4; ++i) {
                    const int k = 4 * (q + 8 * i);
                    const f32x4 gm = *reinterpret_cast<const f32x4*>(s_gb + k), bt = *reinterpret_cast<const f32x4*>(s_gb + K + k);
                    typedef __attribute__((ext_vector_type(4))) unsigned short u16x4;
                    u16x4 oh, om, ol;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float y = (v[i][j] - mean) * rstd * gm[j] + bt[j];  // the fp32 operand the exact kernel multiplies
                        const unsigned uh = __float_as_uint(y) & 0xffff0000u;
                        const float r1 = y - __uint_as_float(uh);
                        const unsigned um = __float_as_uint(r1) & 0xffff0000u;
                        const float r2 = r1 - __uint_as_float(um);
                        oh[j] = (unsigned short)(uh >> 16);
                        om[j] = (unsigned short)(um >> 16);
                        ol[j] = (unsigned short)(__float_as_uint(r2) >> 16);
                    }
                    *reinterpret_cast<u16x4*>(&xs[lr * PITCH + k]) = oh;
                    *reinterpret_cast<u16x4*>(&xs[IMG + lr * PITCH + k]) = om;
                    *reinterpret_cast<u16x4*>(&xs[2 * IMG + lr * PITCH + k]) = ol;
                }
            }
        }
    }
    WM_LG_STAMP(1);
    __syncthreads();
    WM_LG_STAMP(2);
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int i = (nb == 0 ? PRE : 0); i < CHK; ++i) wf[nb][i] = wload(nb, i);

    f32x4 acc[2][NRB];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb) acc[nb][rb] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto body = [&](auto NB) {
        constexpr int nbn = decltype(NB)::value;
#pragma unroll
        for (int c = 0; c < KS / CHK; ++c) {
#pragma unroll
            for (int i = 0; i < CHK; ++i) {
                Split3 ws[nbn];
#pragma unroll
                for (int nb = 0; nb < nbn; ++nb) {
                    ws[nb] = split3(wf[nb][i]);
                    // rolling prefetch: the register set just split takes the same k-step of the next chunk
                    if (c + 1 < KS / CHK) wf[nb][i] = wload(nb, (c + 1) * CHK + i);
                }
#pragma unroll
                for (int rb = 0; rb < NRB; ++rb) {
                    const int xo = (rb * 16 + r16) * PITCH + (c * CHK + i) * 32 + g * 8;
                    const bf16x8 xh = *reinterpret_cast<const bf16x8*>(&xs[xo]);
                    const bf16x8 xm = *reinterpret_cast<const bf16x8*>(&xs[IMG + xo]);
                    const bf16x8 xl = *reinterpret_cast<const bf16x8*>(&xs[2 * IMG + xo]);
#pragma unroll
                    for (int nb = 0; nb < nbn; ++nb) {  // smallest terms first
                        f32x4 a = acc[nb][rb];
                        a = mma_bf16(ws[nb].l, xh, a);
                        a = mma_bf16(ws[nb].h, xl, a);
                        a = mma_bf16(ws[nb].m, xm, a);
                        a = mma_bf16(ws[nb].m, xh, a);
                        a = mma_bf16(ws[nb].h, xm, a);
                        a = mma_bf16(ws[nb].h, xh, a);
                        acc[nb][rb] = a;
                    }
                }
            }
        }
    };
    if (have[1])
        body(std::integral_constant<int, 2>{});
    else if (have[0])
        body(std::integral_constant<int, 1>{});
    WM_LG_STAMP(3);
    __syncthreads();  // every wave is past its last fragment read: the epilogue's scratch overlays the activation images
    static_assert((LP ? LogitsScratch<NRB>::bytes_lp : LogitsScratch<NRB>::bytes) <= (size_t)3 * IMG * sizeof(bf16),
                  "epilogue scratch must fit the activation images");
    logits_epilogue_rp<NRB, LP, RP, SB>(p, CT, acc, n0, have, mk, row0, nrows, lane, w, LogitsScratch<NRB>::carve(smem_raw));
    WM_LG_STAMP(4);
}
#undef WM_LG_STAMP
// The same kernel for 128 rows per workgroup — two coalesced 64-utterance batches on one decode state (wm_config.coalesce): with 64
// rows per workgroup a 128-row state streamed the 80 MB embedding twice per step.  Three bf16 images of 128 x 384 do not fit the
// 160 KB of LDS, so K goes in TWO passes of K/2 columns: stage the first half of every row, multiply it with k-steps 0 .. K/64-1 of
// the workgroup's embedding rows (the second half's weight fragments are requested meanwhile, register set by register set), barrier,
// re-stage, multiply the second half into the same accumulators.  Every row's arithmetic is exactly the 64-row kernel's — the
// LayerNorm statistics are summed in the same order (a thread carries the two partial sums of the two "virtual" threads the
// 8-threads-per-row scheme gives its elements to), the k-steps accumulate in the same order — so the ids of a coalesced pass equal
// the uncoalesced ones bit for bit.
template <int KD /* d_model/128 */, bool LP = false, bool RP = false, bool SB = false>
__global__ __launch_bounds__(512) void dec_logits_split128_kernel(DecLinearParams p, int CT) {
    constexpr int NRB = 8, ROWS = 128;
    constexpr int K = KD * 128, KH = K / 2;  // columns per pass
    constexpr int PITCH = KH + 16;           // ≡ 8 dwords (mod 16): conflict-free fragment reads (see dec_logits_split_kernel)
    constexpr int KSH = KD * 2;              // k-steps of 32 per pass
    constexpr int IMG = ROWS * PITCH;        // elements per image
    constexpr int F4 = K / 16;               // float4 per thread and row (4 threads per row); the first F4/2 belong to pass 0
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    bf16* xs = reinterpret_cast<bf16*>(smem_raw);                                        // [3][128][PITCH]: h, m, l of the current K half
    float* s_gb = reinterpret_cast<float*>(smem_raw + (size_t)3 * IMG * sizeof(bf16));  // [2][K] LN gamma / beta
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int row0 = blockIdx.y * ROWS;
    if (p.ts && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) ts_put(p.ts, p.ts_id, 2);
#ifdef WM_DEV  // phase stamps (wm_bench_kernel id 40): 0 entry, 1 first half staged, 2 past its barrier, 5 first half multiplied, 6 second half staged, 3 all multiplied, 4 end
#define WM_LG_STAMP(k) do { if (p.dbg && (threadIdx.x & 63) == 0) p.dbg[((size_t)blockIdx.x * 8 + (threadIdx.x >> 6)) * 8 + (k)] = (long long)wall_clock64(); } while (0)
#else
#define WM_LG_STAMP(k) do { } while (0)
#endif
    WM_LG_STAMP(0);
    const int nrows = min(ROWS, p.B - row0);
    int n0[2];
    bool have[2];
    const float* wp[2];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const int t = w + 8 * nb;
        n0[nb] = (blockIdx.x * CT + t) * 16;
        have[nb] = __builtin_amdgcn_readfirstlane((int)(t < CT && n0[nb] < p.N)) != 0;
        int wr = n0[nb] + r16;
        wr = wr < p.N ? wr : p.N - 1;
        wp[nb] = (const float*)p.W + (size_t)wr * K + g * 8;
    }
    if (!have[1]) wp[1] = wp[0];
    constexpr int NSL = 3 < 2 * KSH ? 3 : 2 * KSH;  // weight-fragment register sets per tile: k-step kk lives in set kk % NSL and, once
    f32x8 wf[2][NSL];                                // split, the set is refilled with k-step kk + NSL (across the pass boundary too)
    auto wload = [&](int nb, int ks) __attribute__((always_inline)) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(wp[nb] + ks * 32), b = *reinterpret_cast<const f32x4*>(wp[nb] + ks * 32 + 4);
        return f32x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    };
    float mk[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    // staging role: row lr = thread / 4, quarter q4 = thread % 4; the thread owns float4 indices q4 + 4 j (j < F4) of its row
    const int lr = threadIdx.x >> 2, q4 = threadIdx.x & 3;
    const float* xr = p.x + (size_t)(row0 + min(lr, nrows - 1)) * p.ldx;
    float mean, rstd;
    auto stage = [&](const f32x4 (&v)[F4 / 2], int pass) __attribute__((always_inline)) {  // normalise + split the pass's F4/2 float4 of this thread -> LDS
#pragma unroll
        for (int j = 0; j < F4 / 2; ++j) {
            const int k = 4 * (q4 + 4 * (pass * (F4 / 2) + j));  // column of the row
            const f32x4 gm = *reinterpret_cast<const f32x4*>(s_gb + k), bt = *reinterpret_cast<const f32x4*>(s_gb + K + k);
            typedef __attribute__((ext_vector_type(4))) unsigned short u16x4;
            u16x4 oh, om, ol;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float y = (v[j][e] - mean) * rstd * gm[e] + bt[e];
                const unsigned uh = __float_as_uint(y) & 0xffff0000u;
                const float r1 = y - __uint_as_float(uh);
                const unsigned um = __float_as_uint(r1) & 0xffff0000u;
                const float r2 = r1 - __uint_as_float(um);
                oh[e] = (unsigned short)(uh >> 16);
                om[e] = (unsigned short)(um >> 16);
                ol[e] = (unsigned short)(__float_as_uint(r2) >> 16);
            }
            const int kc = k - pass * KH;  // column inside the pass's image
            *reinterpret_cast<u16x4*>(&xs[lr * PITCH + kc]) = oh;
            *reinterpret_cast<u16x4*>(&xs[IMG + lr * PITCH + kc]) = om;
            *reinterpret_cast<u16x4*>(&xs[2 * IMG + lr * PITCH + kc]) = ol;
        }
    };
    {  // pass 0: the whole row for the statistics, its first half staged
        f32x4 v0[F4 / 2], v1[F4 / 2];
#pragma unroll
        for (int j = 0; j < F4 / 2; ++j) {
            v0[j] = *reinterpret_cast<const f32x4*>(xr + 4 * (q4 + 4 * j));
            v1[j] = *reinterpret_cast<const f32x4*>(xr + 4 * (q4 + 4 * (F4 / 2 + j)));
        }
        f32x4 gbv = f32x4{0.f, 0.f, 0.f, 0.f};
        const int gi = threadIdx.x;  // float4 index into [gamma | beta]
        if (gi < K / 2) gbv = *reinterpret_cast<const f32x4*>((gi < K / 4 ? p.ln_g : p.ln_b - K) + 4 * gi);
        if (p.amax_mask) {
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int r = 0; r < 4; ++r) mk[nb][r] = p.amax_mask[min(n0[nb] + g * 4 + r, p.N - 1)];
        }
        if (gi < K / 2) *reinterpret_cast<f32x4*>(s_gb + 4 * gi) = gbv;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NSL; ++i) wf[0][i] = wload(0, i);
        // one-pass statistics in the order of the 8-threads-per-row scheme: virtual thread q owns float4 q + 8 i.  This thread's
        // float4 j is index q4 + 4 j: even j -> virtual thread q4 (i = j / 2), odd j -> virtual thread q4 + 4.
        float sa = 0.f, qa = 0.f, sb = 0.f, qb = 0.f;
        static_assert((F4 / 2) % 2 == 0, "the parity of a float4's index is the same in both halves");
        auto accum = [&](const f32x4 (&v)[F4 / 2]) __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < F4 / 2; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (j & 1) {
                        sb += v[j][e];
                        qb += v[j][e] * v[j][e];
                    } else {
                        sa += v[j][e];
                        qa += v[j][e] * v[j][e];
                    }
                }
        };
        accum(v0);
        accum(v1);
#pragma unroll
        for (int o = 1; o <= 2; o <<= 1) {  // the butterfly's first two levels, inside each half of the 8 virtual threads
            sa += __shfl_xor(sa, o, 64);
            qa += __shfl_xor(qa, o, 64);
            sb += __shfl_xor(sb, o, 64);
            qb += __shfl_xor(qb, o, 64);
        }
        const float sm = sa + sb, sq = qa + qb;  // its last level
        mean = sm / (float)K;
        const float var = (sq / (float)K) - (mean * mean);
        rstd = 1.0f / sqrtf(fmaxf(var, 0.f) + 1e-5f);
        stage(v0, 0);
    }
    WM_LG_STAMP(1);
    __syncthreads();
    WM_LG_STAMP(2);
#pragma unroll
    for (int i = 0; i < NSL; ++i) wf[1][i] = wload(1, i);
    f32x4 acc[2][NRB];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb) acc[nb][rb] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto restage = [&]() __attribute__((always_inline)) {  // every wave, tiles or not: the second K half of the rows
        __syncthreads();  // all fragment reads of the first half are done
        f32x4 v1[F4 / 2];
#pragma unroll
        for (int j = 0; j < F4 / 2; ++j) v1[j] = *reinterpret_cast<const f32x4*>(xr + 4 * (q4 + 4 * (F4 / 2 + j)));
        stage(v1, 1);
        __syncthreads();
    };
    auto run = [&](auto NB) __attribute__((always_inline)) {
        constexpr int nbn = decltype(NB)::value;
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            if (pass == 1) {
                WM_LG_STAMP(5);
                restage();
                WM_LG_STAMP(6);
            }
            if constexpr (nbn > 0) {
#pragma unroll
                for (int i = 0; i < KSH; ++i) {
                    Split3 ws[nbn];
#pragma unroll
                    for (int nb = 0; nb < nbn; ++nb) {
                        constexpr int dummy = 0;
                        (void)dummy;
                        const int kk = pass * KSH + i;  // compile-time after unrolling
                        ws[nb] = split3(wf[nb][kk % NSL]);
                        if (kk + NSL < 2 * KSH) wf[nb][kk % NSL] = wload(nb, kk + NSL);  // rolling: the set just split takes k-step kk + NSL
                    }
                    // Row blocks in pairs, the six products of a k-step interleaved over the pair's (and both tiles') accumulators: 128
                    // rows make this kernel MFMA-bound, and six back-to-back MFMAs on ONE accumulator wait for each other's results.
                    // Per accumulator the order of the six terms is the 64-row kernel's (smallest first).
#pragma unroll
                    for (int rp = 0; rp < NRB; rp += 2) {
                        bf16x8 xh[2], xm[2], xl[2];
#pragma unroll
                        for (int r = 0; r < 2; ++r) {
                            const int xo = ((rp + r) * 16 + r16) * PITCH + i * 32 + g * 8;
                            xh[r] = *reinterpret_cast<const bf16x8*>(&xs[xo]);
                            xm[r] = *reinterpret_cast<const bf16x8*>(&xs[IMG + xo]);
                            xl[r] = *reinterpret_cast<const bf16x8*>(&xs[2 * IMG + xo]);
                        }
#define WM_TERM(WPART, XPART)                                                                            \
    _Pragma("unroll") for (int r = 0; r < 2; ++r) _Pragma("unroll") for (int nb = 0; nb < nbn; ++nb)     \
        acc[nb][rp + r] = mma_bf16(ws[nb].WPART, XPART[r], acc[nb][rp + r]);
                        WM_TERM(l, xh)
                        WM_TERM(h, xl)
                        WM_TERM(m, xm)
                        WM_TERM(m, xh)
                        WM_TERM(h, xm)
                        WM_TERM(h, xh)
#undef WM_TERM
                    }
                }
            }
        }
    };
    if (have[1])
        run(std::integral_constant<int, 2>{});
    else if (have[0])
        run(std::integral_constant<int, 1>{});
    else
        run(std::integral_constant<int, 0>{});
    WM_LG_STAMP(3);
    __syncthreads();  // the epilogue's scratch overlays the activation images
    static_assert((LP ? LogitsScratch<NRB>::bytes_lp : LogitsScratch<NRB>::bytes) <= (size_t)3 * IMG * sizeof(bf16),
                  "epilogue scratch must fit the activation images");
    logits_epilogue_rp<NRB, LP, RP, SB>(p, CT, acc, n0, have, mk, row0, nrows, lane, w, LogitsScratch<NRB>::carve(smem_raw));
    WM_LG_STAMP(4);
}
#undef WM_LG_STAMP
template <int KD, bool LP = false, bool RP = false, bool SB = false> static int launch_dec_logits_split128_t(const DecLinearParams& p, hipStream_t st) {
    const size_t lds = (size_t)3 * 128 * (KD * 64 + 16) * sizeof(bf16) + (size_t)2 * KD * 128 * sizeof(float);
    if (lds > 48 * 1024)
        if (const hipError_t e = ensure_dyn_lds<&dec_logits_split128_kernel<KD, LP, RP, SB>>((int)lds); e != hipSuccess)
            return launch_hip_failed("logits kernel (split fp32, 128 rows): dynamic LDS attribute", e);
    const int ct = dec_logits_tiles_per_wg(p.N);
    dim3 grid(dec_logits_parts(p.N), (p.B + 127) / 128);
    hipLaunchKernelGGL((dec_logits_split128_kernel<KD, LP, RP, SB>), grid, dim3(512), lds, st, p, ct);
    return WM_LAUNCH_OK;
}
template <int KD, int NRB, bool LP = false, bool RP = false, bool SB = false> static int launch_dec_logits_split_t(const DecLinearParams& p, hipStream_t st) {
    const size_t lds = (size_t)3 * NRB * 16 * (KD * 128 + 16) * sizeof(bf16) + (size_t)2 * KD * 128 * sizeof(float);
    if (lds > 48 * 1024)
        if (const hipError_t e = ensure_dyn_lds<&dec_logits_split_kernel<KD, NRB, LP, RP, SB>>((int)lds); e != hipSuccess)
            return launch_hip_failed("logits kernel (split fp32): dynamic LDS attribute", e);
    const int ct = dec_logits_tiles_per_wg(p.N);
    dim3 grid(dec_logits_parts(p.N), (p.B + NRB * 16 - 1) / (NRB * 16));
    hipLaunchKernelGGL((dec_logits_split_kernel<KD, NRB, LP, RP, SB>), grid, dim3(512), lds, st, p, ct);
    return WM_LAUNCH_OK;
}

// column tiles (of 16) per workgroup: the smallest count that covers the vocabulary with <= 256 workgroups, at most 16
int dec_logits_tiles_per_wg(int N) {
    const int tiles = (N + 15) / 16;
    // (developer A/B WM_LOGITS_CT: 14 / 16 tiles per workgroup — every wave two tiles at 16 — measured the same launch time as 13:
    //  the stream's end is set by the chip-wide rate, not by the busiest wave)
    static const int ct_env = wm_env("WM_LOGITS_CT") ? atoi(wm_env("WM_LOGITS_CT")) : 0;
    if (ct_env > 0 && tiles > 16) return std::max((tiles + 255) / 256, std::min(16, ct_env));
    return std::max(1, std::min(16, (tiles + 255) / 256));
}
int dec_logits_ids_per_part(int N) { return dec_logits_tiles_per_wg(N) * 16; }
int dec_logits_parts(int N) {
    const int tiles = (N + 15) / 16, ct = dec_logits_tiles_per_wg(N);
    return (tiles + ct - 1) / ct;
}
template <typename TW, int KD, int NRB, bool LP = false, bool RP = false, bool SB = false> static int launch_dec_logits_t(const DecLinearParams& p, hipStream_t st) {
    constexpr size_t lds = (size_t)NRB * 16 * (KD * 128 + (sizeof(TW) == 2 ? 80 : 16 / sizeof(TW))) * sizeof(TW);
    // beside the image: gamma | beta (8·K bytes) and, up to 64 rows, the epilogue's scratch: 2 x 32 + 4 x 8 (+ 8 with log-probs)
    // floats / ints per row.  At 128 rows the scratch overlays the image.
    static_assert(lds + (size_t)8 * KD * 128 + (NRB <= 4 ? (size_t)NRB * 16 * 4 * (LP ? 104 : 96) : 0) <= 160 * 1024,
                  "activation image + static LDS must fit the 160 KB of a CU");
    if (lds > 48 * 1024)
        if (const hipError_t e = ensure_dyn_lds<&dec_logits_kernel<TW, KD, NRB, LP, RP, SB>>((int)lds); e != hipSuccess)
            return launch_hip_failed("logits kernel: dynamic LDS attribute", e);
    const int ct = dec_logits_tiles_per_wg(p.N);
    dim3 grid(dec_logits_parts(p.N), (p.B + NRB * 16 - 1) / (NRB * 16));
    hipLaunchKernelGGL((dec_logits_kernel<TW, KD, NRB, LP, RP, SB>), grid, dim3(512), lds, st, p, ct);
    return WM_LAUNCH_OK;
}
// requires ln_g/ln_b, no bias/act/residual, K in {128, 384, 512, 768, 1024}, ldo % 4 == 0; amax_stride >= dec_logits_parts(N)
template <typename TW, bool LP, bool RP, bool SB> static int launch_dec_logits_lp(const DecLinearParams& p, hipStream_t st) {
    const int kd = p.K >> 7;
    if (p.B <= 0 || p.N <= 0) return launch_refuse("dec_logits: empty problem");
    if ((p.K & 127) != 0 || (kd != 1 && kd != 3 && kd != 4 && kd != 6 && kd != 8)) return launch_refuse("dec_logits: d_model must be 128, 384, 512, 768 or 1024");
    if (!p.ln_g || !p.ln_b) return launch_refuse("dec_logits: the final LayerNorm's gamma / beta are required");
    if (p.amax_val && p.amax_stride < dec_logits_parts(p.N)) return launch_refuse("dec_logits: amax_stride is smaller than the partials per utterance");
    if (LP && !p.amax_val) return launch_refuse("dec_logits: log-probabilities need the fused argmax (amax_val)");
    if constexpr (sizeof(TW) == 4) {
        // fp32 weights: the three-way bf16 split (d_model 128 / 384: three activation images fit the 160 KB of LDS); d_model 512
        // keeps the exact-fp32 MFMA kernel, and so does d_model 768 — NOT the split: three bf16 images of 64 x 768 are 301 KB.  At 768
        // even one fp32 image of 64 rows (64 x 772 x 4 = 198 KB) is past the LDS, so the exact kernel runs 32 rows per workgroup there
        // (99 KB) and a 64- or 128-row state is 2 or 4 row blocks in grid.y: the kernel is MFMA-bound with fp32 operands (see the note
        // at dec_logits_split_kernel), the MFMA count is the same, and the embedding's second read comes from the Infinity Cache.  A
        // row's arithmetic does not depend on the rows beside it, so ids stay bitwise equal across batch sizes and coalescing.
        // WM_LOGITS_EXACT (developer build) forces the exact kernel for A/B runs.
        static const bool exact = wm_env("WM_LOGITS_EXACT") != nullptr;
        if (!exact && (kd == 1 || kd == 3)) {
            if (p.B <= 16) return kd == 1 ? launch_dec_logits_split_t<1, 1, LP, RP, SB>(p, st) : launch_dec_logits_split_t<3, 1, LP, RP, SB>(p, st);
            // more than 64 rows (coalesced batches): 128 rows per workgroup, the embedding streamed once per 128 (WM_LOGITS_NO128: A/B)
            static const bool no128 = wm_env("WM_LOGITS_NO128") != nullptr;
            if (p.B > 64 && !no128) return kd == 1 ? launch_dec_logits_split128_t<1, LP, RP, SB>(p, st) : launch_dec_logits_split128_t<3, LP, RP, SB>(p, st);
            return kd == 1 ? launch_dec_logits_split_t<1, 4, LP, RP, SB>(p, st) : launch_dec_logits_split_t<3, 4, LP, RP, SB>(p, st);
        }
    }
    if (p.B <= 16) {
        if (kd == 1) return launch_dec_logits_t<TW, 1, 1, LP, RP, SB>(p, st);
        if (kd == 3) return launch_dec_logits_t<TW, 3, 1, LP, RP, SB>(p, st);
        if (kd == 6) return launch_dec_logits_t<TW, 6, 1, LP, RP, SB>(p, st);
        if (kd == 8) return launch_dec_logits_t<TW, 8, 1, LP, RP, SB>(p, st);
        return launch_dec_logits_t<TW, 4, 1, LP, RP, SB>(p, st);
    }
    // d_model 1024: 32 rows per workgroup for every operand type (16-bit: 32 x 1104 x 2 = 69 KB image + 21 KB static; fp32:
    // 32 x 1028 x 4 = 129 KB + 21 KB; 64 rows of 16-bit would be 138 + 34 KB, past the 160).  More rows are more row blocks in grid.y.
    if (kd == 8) return launch_dec_logits_t<TW, 8, 2, LP, RP, SB>(p, st);
    if (kd == 6) return launch_dec_logits_t<TW, 6, sizeof(TW) == 4 ? 2 : 4, LP, RP, SB>(p, st);  // (16-bit, 64 rows: 106 KB image + 30 KB static)
#ifdef WM_DEV
    if constexpr (sizeof(TW) == 2) {
        // Developer A/B (WM_LOGITS_128_16BIT): 128 rows per workgroup for 16-bit weights too.  Measured SLOWER than two 64-row
        // launches (tiny bf16, coalesced pairs: 16.5 vs 15.8 ms per pass; base f16: equal): the second launch's 40 MB embedding
        // stream is served by the Infinity Cache, so there is no HBM traffic to save, and the 128-row form stages and reduces twice
        // the rows behind one stream.  The fp32 form (80 MB per stream, MFMA-heavy) does gain: dec_logits_split128_kernel.
        static const bool on128 = wm_env("WM_LOGITS_128_16BIT") != nullptr;
        if (p.B > 64 && on128) {
            if (kd == 1) return launch_dec_logits_t<TW, 1, 8, LP, RP, SB>(p, st);
            if (kd == 3) return launch_dec_logits_t<TW, 3, 8, LP, RP, SB>(p, st);
            return launch_dec_logits_t<TW, 4, 8, LP, RP, SB>(p, st);
        }
    }
#endif
    if (kd == 1) return launch_dec_logits_t<TW, 1, 4, LP, RP, SB>(p, st);
    if (kd == 3) return launch_dec_logits_t<TW, 3, 4, LP, RP, SB>(p, st);
    return launch_dec_logits_t<TW, 4, 4, LP, RP, SB>(p, st);
}
// p.lp_s null: exactly the kernels, grids and LDS of a pass without log-probabilities; non-null: the LP instantiation of the same variant
// p.rp_seen likewise: null is the pass without the repetition processors, non-null the RP instantiation of the same variant
template <typename TW> int launch_dec_logits(const DecLinearParams& p, hipStream_t st) {
    if (p.rp_seen) {
        if (!p.rp_ban || !p.rp_ctl || p.rp_words < repeat_words(p.N)) return launch_refuse("dec_logits: the repetition processors need both sets of ceil(N / 32) words per row and their control block");
        if (p.sb_hit) {  // sequence bias / bad words: the SB instantiation of the same variant
            if (!p.sb_val || !p.sb_ctl) return launch_refuse("dec_logits: the sequence bias needs the rows' slots and the control block");
            return p.lp_s ? launch_dec_logits_lp<TW, true, true, true>(p, st) : launch_dec_logits_lp<TW, false, true, true>(p, st);
        }
        return p.lp_s ? launch_dec_logits_lp<TW, true, true, false>(p, st) : launch_dec_logits_lp<TW, false, true, false>(p, st);
    }
    if (p.sb_hit) return launch_refuse("dec_logits: the sequence bias needs the repetition processors' sets (penalty 1, n-gram 0 = no-ops)");
    return p.lp_s ? launch_dec_logits_lp<TW, true, false, false>(p, st) : launch_dec_logits_lp<TW, false, false, false>(p, st);
}
template int launch_dec_logits<float>(const DecLinearParams&, hipStream_t);
template int launch_dec_logits<bf16>(const DecLinearParams&, hipStream_t);
template int launch_dec_logits<f16>(const DecLinearParams&, hipStream_t);

// ------------------------------------------------------------------------------------------------------------
// Single-query attention over the KV cache (layers.mojo:186-272), all heads of one utterance per workgroup so that
// whole token-major cache rows (H*64 elements, the reference's layout: layers.mojo:140-147) stream fully coalesced.
// grid = (nsplit key chunks, B).  Lane map: LPH lanes (16 B each) cover one head's 64 dims of one key; LPR = H*LPH
// lanes cover a row; the block sweeps RPS rows per step, U steps per iteration.
// ONE pass: K and V rows of an iteration are requested together (and the next iteration's before this one is
// consumed), scores reduce inside an aligned LPH-lane group with DPP only, and the softmax is the online form
// (running max / sum per lane, one rescale per iteration) — every K and V byte is read once, nothing is parked in LDS
// except the final merge of the RPS row slots.  Emits un-normalised partials (o, max, sum) per chunk for
// attn_combine, or the normalised output directly when the chunk is the whole sequence.
// Scale after the dot product and max initialised to -1e10 follow layers.mojo:196,212 (the mask branch at :213 is a
// no-op for j <= len-1 and is omitted).
// LO (per-row prompts, self-attention forms only): utterance bk sweeps keys [key_lo[bk], len) instead of [0, len) — the rows of a pass
// are aligned at the END of the longest prompt, so a shorter prompt has dead cache rows in front.  The sweep starts AT key_lo (row
// slot r takes keys key_lo + r, key_lo + r + RPS, ...): a row's arithmetic is what it would be alone with its own unpadded prompt.
// An empty window (a dead prefill slot) stores zeros.  LO = false is the kernel as it always was.
// MAP (n-best scoring; cross-attention forms only): the K/V this workgroup reads are those of utt_of[bq] instead of bq —
// several query rows share one clip's K/V.  Queries, outputs and every sum are the row's own: MAP = false is the kernel as it always was.
template <typename TKV, int LPH, bool FAST, bool NT, int U, int NQ, bool LO, bool MAP = false>
__device__ __forceinline__ void attn_decode_body(const AttnDecParams& p, const int* __restrict__ key_lo, const int* __restrict__ utt_of = nullptr) {
    // NQ > 1 (prompt prefill, cross-attention): the workgroup of utterance b serves the NQ query rows t * B + b from ONE
    // sweep of that utterance's K/V chunk — each cache row is read once for all prompt positions.
    constexpr int EPL = 64 / LPH;  // elements per lane
    __shared__ float s_ml[512][2];
    __shared__ float s_red[512 * EPL];
    const int b = blockIdx.y, split = blockIdx.x;
    if (p.ts && NT && b == 0 && split == 0 && threadIdx.x == 0) ts_put(p.ts, p.ts_id, 0);
    const int LPR = p.H * LPH;
    const int RPS = p.rps;  // key rows swept per step = active threads / LPR
    const int bq = (NQ == 1 && p.q_B > 0) ? b % p.q_B : b;  // the row's slot in the batch
    const int bk = MAP ? utt_of[bq] : bq;  // utterance whose K/V this workgroup reads
    const int len = p.n_keys >= 0 ? p.n_keys : p.ctl->len + 1 + ((NQ == 1 && p.q_B > 0) ? b / p.q_B : 0);  // (scalar chain kernarg -> ctl -> len: the loop bounds need it before any K/V row is requested)
    const int qstride = NQ > 1 ? p.q_B : 0;  // query / output row of position t: b + t * qstride
    const int lo = LO ? key_lo[bk] : 0;
    const int chunk = LO ? max(len - lo, 0) : (len + p.nsplit - 1) / p.nsplit;  // (LO: nsplit == 1)
    const int j0 = lo + split * chunk;
    const int j1 = min(len, j0 + chunk);
    const int rslot = threadIdx.x / LPR, c = threadIdx.x % LPR;
    const int h = c / LPH, e0 = (c % LPH) * EPL;
    const bool active = rslot < RPS;

    float qv[NQ][EPL];
#pragma unroll
    for (int t = 0; t < NQ; ++t)
#pragma unroll
        for (int e = 0; e < EPL; ++e) qv[t][e] = p.q[(size_t)(b + t * qstride) * p.d + h * 64 + e0 + e] * p.scale;
    const TKV* Kb = (const TKV*)p.K + (size_t)bk * p.batch_stride + h * 64 + e0;
    const TKV* Vb = (const TKV*)p.V + (size_t)bk * p.batch_stride + h * 64 + e0;
    typedef __attribute__((ext_vector_type(EPL))) TKV kvec;

    float m_run[NQ], l_run[NQ];
    float acc[NQ][EPL];
#pragma unroll
    for (int t = 0; t < NQ; ++t) {
        m_run[t] = -1e10f;
        l_run[t] = 0.f;
#pragma unroll
        for (int e = 0; e < EPL; ++e) acc[t][e] = 0.f;
    }
    const int step = RPS * U;

    auto load = [&](kvec (&kk)[U], kvec (&vv)[U], int j) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int jj = max(min(j + u * RPS, j1 - 1), 0);
            if (NT) {  // read-once stream: keep it out of L2 / Infinity Cache so the weights stay resident there
                kk[u] = __builtin_nontemporal_load(reinterpret_cast<const kvec*>(Kb + (size_t)jj * p.d));
                vv[u] = __builtin_nontemporal_load(reinterpret_cast<const kvec*>(Vb + (size_t)jj * p.d));
            } else {
                kk[u] = *reinterpret_cast<const kvec*>(Kb + (size_t)jj * p.d);
                vv[u] = *reinterpret_cast<const kvec*>(Vb + (size_t)jj * p.d);
            }
        }
    };
    auto consume = [&](const kvec (&kk)[U], const kvec (&vv)[U], int j) {
#pragma unroll
        for (int t = 0; t < NQ; ++t) {
            float sc[U];
            float bm = -1e30f;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float dot = 0.f;
#pragma unroll
                for (int e = 0; e < EPL; ++e) dot += qv[t][e] * (float)kk[u][e];
                dot = LPH == 16 ? group_sum16(dot) : group_sum8(dot);
                sc[u] = (active && j + u * RPS < j1) ? dot : -1e30f;
                bm = fmaxf(bm, sc[u]);
            }
            const float m_new = fmaxf(m_run[t], bm);
            const float alpha = FAST ? __expf(m_run[t] - m_new) : expf(m_run[t] - m_new);
            float ps = 0.f;
#pragma unroll
            for (int e = 0; e < EPL; ++e) acc[t][e] *= alpha;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float pe = FAST ? __expf(sc[u] - m_new) : expf(sc[u] - m_new);
                ps += pe;
#pragma unroll
                for (int e = 0; e < EPL; ++e) acc[t][e] += pe * (float)vv[u][e];
            }
            l_run[t] = l_run[t] * alpha + ps;
            m_run[t] = m_new;
        }
    };

    {
        kvec ka[U], va[U], kb[U], vb[U];
        int j = j0 + rslot;
        if (j0 < j1) {
            load(ka, va, j);
            while (true) {
                const bool more1 = j + step < j1 + RPS;  // some row slot still has keys in the next iteration
                if (more1) load(kb, vb, j + step);
                consume(ka, va, j);
                j += step;
                if (!more1) break;
                const bool more2 = j + step < j1 + RPS;
                if (more2) load(ka, va, j + step);
                consume(kb, vb, j);
                j += step;
                if (!more2) break;
            }
        }
    }
    // merge the RPS row slots (lanes of one LPH group carry identical m, l), one query position after the other
#pragma unroll
    for (int t = 0; t < NQ; ++t) {
        if (t > 0) __syncthreads();  // everyone is done reading the previous position's partials
        s_ml[threadIdx.x][0] = m_run[t];
        s_ml[threadIdx.x][1] = l_run[t];
#pragma unroll
        for (int e = 0; e < EPL; ++e) s_red[threadIdx.x * EPL + e] = acc[t][e];
        __syncthreads();
        if (rslot == 0) {
            float M = -1e10f;
            for (int r = 0; r < RPS; ++r) M = fmaxf(M, s_ml[r * LPR + c][0]);
            float L = 0.f, o[EPL];
#pragma unroll
            for (int e = 0; e < EPL; ++e) o[e] = 0.f;
            for (int r = 0; r < RPS; ++r) {
                const int tt = r * LPR + c;
                const float wgt = s_ml[tt][1] > 0.f ? (FAST ? __expf(s_ml[tt][0] - M) : expf(s_ml[tt][0] - M)) : 0.f;
                L += wgt * s_ml[tt][1];
#pragma unroll
                for (int e = 0; e < EPL; ++e) o[e] += wgt * s_red[tt * EPL + e];
            }
            const size_t orow = (size_t)b + (size_t)t * qstride;
            if (p.direct_out) {
                const float norm = (LO && !(L > 0.f)) ? 0.f : 1.0f / L;
#pragma unroll
                for (int e = 0; e < EPL; ++e) store_as(p.direct_out, orow * p.d + h * 64 + e0 + e, o[e] * norm, p.out_dtype);
            } else {
                float* po = p.part_o + (orow * p.nsplit + split) * p.d + h * 64 + e0;
#pragma unroll
                for (int e = 0; e < EPL; ++e) po[e] = o[e];
            }
            if (!p.direct_out && (c % LPH) == 0) {
                float* pml = p.part_ml + ((orow * p.nsplit + split) * p.H + h) * 2;
                pml[0] = M;
                pml[1] = L;
            }
        }
    }
}
template <typename TKV, int LPH, bool FAST, bool NT, int U, int NQ = 1>
__global__ __launch_bounds__(512) void attn_decode_kernel(AttnDecParams p) {
    attn_decode_body<TKV, LPH, FAST, NT, U, NQ, false>(p, nullptr);
}
template <typename TKV, int LPH, bool FAST, int U>
__global__ __launch_bounds__(512) void attn_decode_lo_kernel(AttnDecParams p, const int* __restrict__ key_lo) {
    attn_decode_body<TKV, LPH, FAST, false, U, 1, true>(p, key_lo);
}
// the cross-attention forms (nq = 4 or one query per workgroup) with the K/V of utt_of[slot].  Never the non-temporal loads of the
// forms it mirrors: the rows of one clip re-read its K/V, so the stream is not read-once (loads only: the arithmetic is the same).
template <typename TKV, int LPH, bool FAST, int U, int NQ>
__global__ __launch_bounds__(512) void attn_decode_map_kernel(AttnDecParams p, const int* __restrict__ utt_of) {
    attn_decode_body<TKV, LPH, FAST, false, U, NQ, false, true>(p, nullptr, utt_of);
}
template <typename TKV> int launch_attn_decode(const AttnDecParams& p, hipStream_t st, const int* key_lo, const int* utt_of) {
    constexpr int LPH = sizeof(TKV) == 4 ? 16 : 8;
    constexpr bool FAST = sizeof(TKV) == 2;
    const int LPR = p.H * LPH;
    if (p.B <= 0 || p.H <= 0 || LPR > 256 || p.d != p.H * 64) return launch_refuse("attn_decode: needs 1 <= heads <= 16 of 64 dims (d = 64 heads)");
    if (p.nsplit < 1 || (!p.direct_out && (!p.part_o || !p.part_ml)) || (p.direct_out && p.nsplit != 1))
        return launch_refuse("attn_decode: partial buffers / direct output do not match nsplit");
    AttnDecParams q = p;
    // rows swept per step.  16-bit K/V: 256 threads (512 measured no better for the short self-attention: 5.3 vs 5.0 us).
    // fp32 K/V rows are twice as wide (96-128 lanes per row): the latency-bound self-attention takes 512 threads so a
    // lane's serial key loop stays short (61 keys: 16 -> 7 iterations)
    q.rps = ((sizeof(TKV) == 4 && p.n_keys < 0) ? 512 : 256) / LPR;
    static const int thr_self = wm_env("WM_SELF_THREADS") ? atoi(wm_env("WM_SELF_THREADS")) : 0;  // A/B: self-attention block size
    if (thr_self && p.n_keys < 0) q.rps = std::max(1, std::min(512, thr_self) / LPR);
    static const int thr_cross = wm_env("WM_ATTN_THREADS") ? atoi(wm_env("WM_ATTN_THREADS")) : 0;  // A/B: cross-attention block size
    if (thr_cross && p.n_keys >= 0) q.rps = std::max(1, std::min(512, thr_cross) / LPR);
    // block rounded up to whole waves: the spare lanes take no rows (rslot >= RPS) but stay in the DPP groups
    const dim3 grid(p.nsplit, p.B), block((q.rps * LPR + 63) / 64 * 64);
    if (key_lo) {  // per-row prompts: the self-attention forms with a key window
        if (p.n_keys >= 0 || !p.direct_out || p.nq > 1) return launch_refuse("attn_decode: key_lo belongs to the single-workgroup self-attention forms");
        hipLaunchKernelGGL((attn_decode_lo_kernel<TKV, LPH, FAST, 4>), grid, block, 0, st, q, key_lo);
        return WM_LAUNCH_OK;
    }
    if (utt_of) {  // n-best scoring: the chunked cross-attention forms, K/V by row map (same grid, block and U as the forms below)
        if (p.n_keys < 0 || p.direct_out) return launch_refuse("attn_decode: utt_of belongs to the chunked cross-attention forms");
        if (p.nq == 4) {
            hipLaunchKernelGGL((attn_decode_map_kernel<TKV, LPH, FAST, 4, 4>), dim3(p.nsplit, p.q_B), block, 0, st, q, utt_of);
            return WM_LAUNCH_OK;
        }
        static const int map_pad_env = wm_env("WM_ATTN_LDS_PAD") ? atoi(wm_env("WM_ATTN_LDS_PAD")) : -1;  // dev A/B override, as below
        const int map_pad = map_pad_env >= 0 ? map_pad_env : p.lds_pad;
        if (map_pad > 40 * 1024)
            if (const hipError_t e = ensure_dyn_lds<&attn_decode_map_kernel<TKV, LPH, FAST, 4, 1>>(map_pad); e != hipSuccess)
                return launch_hip_failed("attn_decode: dynamic LDS attribute", e);
        hipLaunchKernelGGL((attn_decode_map_kernel<TKV, LPH, FAST, 4, 1>), grid, block, map_pad, st, q, utt_of);
        return WM_LAUNCH_OK;
    }
    static const bool nt_off = wm_env("WM_NO_NT") != nullptr;
    static const int u_cross = wm_env("WM_ATTN_U") ? atoi(wm_env("WM_ATTN_U")) : 4;
    if (p.n_keys >= 0 && p.nq == 4) {  // prompt prefill, four positions per utterance from one K/V sweep (q_B = utterances)
        const dim3 grid4(p.nsplit, p.q_B);
        hipLaunchKernelGGL((attn_decode_kernel<TKV, LPH, FAST, true, 4, 4>), grid4, block, 0, st, q);  // U = 4 as in the step kernel: same arithmetic per query
        return WM_LAUNCH_OK;
    }
    if (p.n_keys >= 0 && !nt_off) {  // the cross-attention K/V stream (1500 rows per utterance, read once per step)
        // p.lds_pad: unused dynamic LDS that caps the workgroups per CU (160 KB / (20 KB static + pad)) — see AttnDecParams
        static const int pad_env = wm_env("WM_ATTN_LDS_PAD") ? atoi(wm_env("WM_ATTN_LDS_PAD")) : -1;  // dev A/B override
        const int lds_pad = pad_env >= 0 ? pad_env : p.lds_pad;
        if (lds_pad > 40 * 1024)
            if (const hipError_t e = ensure_dyn_lds<&attn_decode_kernel<TKV, LPH, FAST, true, 4>>(lds_pad); e != hipSuccess)
                return launch_hip_failed("attn_decode: dynamic LDS attribute", e);
#ifdef WM_DEV
        if (u_cross == 8) {
            hipLaunchKernelGGL((attn_decode_kernel<TKV, LPH, FAST, true, 8>), grid, block, 0, st, q);
            return WM_LAUNCH_OK;
        } else if (u_cross == 2) {
            hipLaunchKernelGGL((attn_decode_kernel<TKV, LPH, FAST, true, 2>), grid, block, 0, st, q);
            return WM_LAUNCH_OK;
        }
#endif
        (void)u_cross;
        hipLaunchKernelGGL((attn_decode_kernel<TKV, LPH, FAST, true, 4>), grid, block, lds_pad, st, q);
    } else {
        // self-attention: 4 rows per lane per iteration (measured per 64-clip pass alone: U = 1 / 2 34.6 ms, U = 4 34.3 ms — the
        // serial iteration count matters as the cache grows to 104 rows).  WM_SELF_U=2 for A/B.
#ifdef WM_DEV
        static const int u_self = wm_env("WM_SELF_U") ? atoi(wm_env("WM_SELF_U")) : 4;
        if (u_self == 2) {
            hipLaunchKernelGGL((attn_decode_kernel<TKV, LPH, FAST, false, 2>), grid, block, 0, st, q);
            return WM_LAUNCH_OK;
        }
#endif
        hipLaunchKernelGGL((attn_decode_kernel<TKV, LPH, FAST, false, 4>), grid, block, 0, st, q);
    }
    return WM_LAUNCH_OK;
}
template int launch_attn_decode<float>(const AttnDecParams&, hipStream_t, const int*, const int*);
template int launch_attn_decode<bf16>(const AttnDecParams&, hipStream_t, const int*, const int*);
template int launch_attn_decode<f16>(const AttnDecParams&, hipStream_t, const int*, const int*);

// merge the key-chunk partials: out[b][h*64+e] = Σ_s w_s·o_s / Σ_s w_s·l_s,  w_s = exp(m_s − max m).
// One wave per (utterance, head): lane s owns chunk s's (m, l) — one exp per chunk, not per element — and the
// weights reach the 64 output lanes by wave broadcast.  nsplit <= 64.
__global__ void attn_combine_kernel(const float* __restrict__ part_o, const float* __restrict__ part_ml,
                                    void* __restrict__ out, int out_dtype, int nsplit, int H, int d, long long* ts, int ts_id) {
    const int b = blockIdx.x, lane = threadIdx.x & 63, h = threadIdx.x >> 6;
    if (ts && b == 0 && threadIdx.x == 0) ts_put(ts, ts_id, 1);
    float m = -1e30f, l = 0.f;
    if (lane < nsplit) {
        const float* ml = part_ml + (((size_t)b * nsplit + lane) * H + h) * 2;
        m = ml[0];
        l = ml[1];
    }
    const float M = wave_max(l > 0.f ? m : -1e30f);
    const float wgt = l > 0.f ? expf(m - M) : 0.f;
    const float L = wave_sum(wgt * l);
    const float* po = part_o + (size_t)b * nsplit * d + h * 64 + lane;
    float o = 0.f;
    int s = 0;
    for (; s + 8 <= nsplit; s += 8) {  // 8 independent loads in flight
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = po[(size_t)(s + j) * d];
#pragma unroll
        for (int j = 0; j < 8; ++j) o += __shfl(wgt, s + j, 64) * v[j];
    }
    for (; s < nsplit; ++s) o += __shfl(wgt, s, 64) * po[(size_t)s * d];
    store_as(out, (size_t)b * d + h * 64 + lane, o * (1.0f / L), out_dtype);
}
void launch_attn_combine(const float* part_o, const float* part_ml, void* out, int out_dtype, int B, int nsplit, int H, int d,
                         hipStream_t st, long long* ts, int ts_id) {
    hipLaunchKernelGGL(attn_combine_kernel, dim3(B), dim3(64 * H), 0, st, part_o, part_ml, out, out_dtype, nsplit, H, d, ts, ts_id);
}

// ------------------------------------------------------------------------------------------------------------
// Cross-attention over the encoder output X (bf16 encoder operands, fp32 K/V): the K/V projections are absorbed into the
// query and the output instead of being materialised as an fp32 cache.  For head h (Wk has no bias; bv is added after the
// softmax average because the weights sum to one):
//     s_hj = (scale·q_h)·(Wk_h·X_j) = q'_h·X_j,   q'_h = (scale·q_h)·Wk_h            (a d-vector per head)
//     o_h  = Σ_j p_hj (Wv_h·X_j + bv_h) / l_h = ((Σ_j p_hj X_j) / l_h)·Wv_hᵀ + bv_h
// X is the projection's own bf16 operand, so the step streams n_keys·d·2 bytes per utterance and layer instead of
// 2·n_keys·d·4: a quarter of the bytes.  Every product is still an exact product of a bf16 value with an fp32 value
// (the fp32 factor carried as three bf16 terms, h + m + l, which reproduce it exactly in the normal range); only the
// order of the fp32 roundings differs from the cached form.

// fp32 -> three bf16 by truncation: x = h + m + l exactly (8 + 8 + 8 significant bits; as split3 above)
__device__ __forceinline__ void split3_1(float x, unsigned short& h, unsigned short& m, unsigned short& l) {
    const unsigned uh = __float_as_uint(x) & 0xffff0000u;
    const float r1 = x - __uint_as_float(uh);
    const unsigned um = __float_as_uint(r1) & 0xffff0000u;
    const float r2 = r1 - __uint_as_float(um);
    h = (unsigned short)(uh >> 16);
    m = (unsigned short)(um >> 16);
    l = (unsigned short)(__float_as_uint(r2) >> 16);
}

// q'[row][h][c] = Σ_e (scale·q[row][h*64+e])·Wk[h*64+e][c], written once per row as three bf16 images [row][3][H][d].
// grid (ceil(rows / 4), H), d/2 threads: thread t owns columns 2t, 2t+1 of four rows (one coalesced Wk row read per e).
// EARLY: the thread's 64 Wk loads depend on nothing loaded, so all of them are requested before q is loaded, staged and the barrier
// passed — one memory round trip under the staging instead of four batches of 16 after it.  The e loop then runs on the registers:
// same order, same fmafs, bitwise the same images.  EARLY = false is the loop as it was (op tests, A/B).
template <bool EARLY>
__global__ __launch_bounds__(256) void xattn_absorb_kernel(XAttnParams p) {
    constexpr int R = 4;
    __shared__ float sq[R][64];
    const int r0 = blockIdx.x * R, h = blockIdx.y, t = threadIdx.x;
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
    const bf16* w = (const bf16*)p.Wk + (size_t)h * 64 * p.d + 2 * t;
    bf16x2 wr[EARLY ? 64 : 1];
    if constexpr (EARLY) {
#pragma unroll
        for (int e = 0; e < 64; ++e) wr[e] = *reinterpret_cast<const bf16x2*>(w + (size_t)e * p.d);
    }
    for (int i = t; i < R * 64; i += blockDim.x) {
        const int r = r0 + i / 64;
        sq[i / 64][i % 64] = r < p.rows ? p.q[(size_t)r * p.d + h * 64 + i % 64] * p.scale : 0.f;
    }
    __syncthreads();
    float acc[R][2];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r][0] = acc[r][1] = 0.f;
    if constexpr (EARLY) {
#pragma unroll
        for (int e = 0; e < 64; ++e) {
            const float w0 = (float)wr[e][0], w1 = (float)wr[e][1];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                acc[r][0] = fmaf(sq[r][e], w0, acc[r][0]);
                acc[r][1] = fmaf(sq[r][e], w1, acc[r][1]);
            }
        }
    } else {
#pragma unroll 16
        for (int e = 0; e < 64; ++e) {
            const bf16x2 wv = *reinterpret_cast<const bf16x2*>(w + (size_t)e * p.d);
            const float w0 = (float)wv[0], w1 = (float)wv[1];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                acc[r][0] = fmaf(sq[r][e], w0, acc[r][0]);
                acc[r][1] = fmaf(sq[r][e], w1, acc[r][1]);
            }
        }
    }
    unsigned short* qs = (unsigned short*)p.qs;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (r0 + r >= p.rows) break;
        unsigned short hh[2], mm[2], ll[2];
        split3_1(acc[r][0], hh[0], mm[0], ll[0]);
        split3_1(acc[r][1], hh[1], mm[1], ll[1]);
        const size_t img = (size_t)p.H * p.d, base = (size_t)(r0 + r) * 3 * img + (size_t)h * p.d + 2 * t;
        *reinterpret_cast<unsigned*>(qs + base) = hh[0] | ((unsigned)hh[1] << 16);
        *reinterpret_cast<unsigned*>(qs + base + img) = mm[0] | ((unsigned)mm[1] << 16);
        *reinterpret_cast<unsigned*>(qs + base + 2 * img) = ll[0] | ((unsigned)ll[1] << 16);
    }
}

// The X sweep.  grid (nsplit key chunks, rows), 4 waves; each wave takes every 4th 16-key tile of the chunk.
//   S (16 keys x 16 columns = heads, columns >= H read a zero row) = X_tile · q'ᵀ: per 32-dim k-step three
//     v_mfma_f32_16x16x32_bf16 (q' = h + m + l) into one accumulator; A = X rows straight from global memory (16 B per lane).
//   online softmax per head as attn_decode_kernel: running max from -1e10, scale already inside q', expf.
//   Yᵀ (d x heads) += X_tileᵀ · P: the tile is parked row-major in the wave's LDS slice and read back transposed with
//     ds_read_b64_tr_b16 (lane (dim r16, group g) gets keys 4g..4g+3 — exactly the keys its P fragment holds, the C map of S);
//     P = h + m + l as three v_mfma_f32_16x16x16_bf16.
// The four waves' (Y, m, l) are merged through LDS and leave as one un-normalised partial per chunk.
typedef __attribute__((ext_vector_type(4))) short s16x4;
__device__ __forceinline__ f32x4 mma16_bf16(const bf16x4& a, const bf16x4& b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s16x4, a), __builtin_bit_cast(s16x4, b), c, 0, 0, 0);
}
__device__ __forceinline__ bf16x4 lds_tr16_bf16(const bf16* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)p);
}
__device__ __forceinline__ void wave_lds_fence() {  // this wave's LDS writes / reads are ordered against its next ones
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

template <int H, bool NT>
__global__ __launch_bounds__(256, 2) void xattn_kernel(XAttnParams p) {
#define XATTN_UTT(slot) slot
#include "xattn_sweep.inc"
#undef XATTN_UTT
}
// The same sweep with X by row map (n-best scoring): the row in batch slot b sweeps the X of clip utt_of[b].  Rows of one
// clip re-read its X, so never the non-temporal form.
template <int H>
__global__ __launch_bounds__(256, 2) void xattn_map_kernel(XAttnParams p, const int* __restrict__ utt_of) {
    constexpr bool NT = false;
#define XATTN_UTT(slot) utt_of[slot]
#include "xattn_sweep.inc"
#undef XATTN_UTT
}

// Merge the chunk partials of one head (exactly attn_combine_kernel's weights) and apply Wv_h: out[row][h*64+e] =
// y_h·Wv[h*64+e]ᵀ + bv[h*64+e].  grid (ceil(rows / 4), H), 256 threads: four rows per workgroup share each Wv row read.
__global__ __launch_bounds__(256) void xattn_merge_kernel(XAttnParams p) {
    constexpr int R = 4, DMAX = 512, NSP = 2, NI = R * DMAX / 4 / 256;
    __shared__ __attribute__((aligned(16))) float sy[R][DMAX];
    __shared__ float sw[R][64], sL[R];
    const int r0 = blockIdx.x * R, h = blockIdx.y, t = threadIdx.x, D = p.d, H = p.H, ns = p.nsplit;
    // Everything is requested before anything is waited for (no address depends on loaded data): the (m, l) pairs, the partials
    // of the first NSP chunks (all of them at the model paths' 1-2 chunks) and this thread's Wv fragments — one memory round trip
    // where the reduce -> barrier -> combine -> barrier -> V-apply order made three.
    const int wr = t >> 6, lane = t & 63;  // chunk weights of row r0 + wr, one wave per row
    float m = -1e30f, l = 0.f;
    if (r0 + wr < p.rows && lane < ns) {
        const float* ml = p.part_ml + (((size_t)(r0 + wr) * ns + lane) * H + h) * 2;
        m = ml[0];
        l = ml[1];
    }
    f32x4 yv[NI][NSP];
#pragma unroll
    for (int k = 0; k < NI; ++k) {
        const int j = t + 256 * k, r = j / (D / 4), c = (j % (D / 4)) * 4;
        if (j < R * (D / 4) && r0 + r < p.rows) {
            const float* py = p.part_y + ((size_t)(r0 + r) * ns * H + h) * D + c;
#pragma unroll
            for (int s = 0; s < NSP; ++s)
                if (s < ns) yv[k][s] = *reinterpret_cast<const f32x4*>(py + (size_t)s * H * D);
        }
    }
    // V-apply: four lanes per output feature e, interleaved over c so that they read 64 contiguous bytes of the Wv row per load
    // (one lane per whole Wv row, 64 rows per load, measured 14.4 us per launch at 128 rows)
    const int e = t >> 2, q = t & 3;
    const bf16* wv = (const bf16*)p.Wv + (size_t)(h * 64 + e) * D;
    bf16x8 wf[DMAX / 32];
#pragma unroll
    for (int it = 0; it < DMAX / 32; ++it)
        if (it < D / 32) wf[it] = *reinterpret_cast<const bf16x8*>(wv + (it * 4 + q) * 8);
    {
        const float M = wave_max(l > 0.f ? m : -1e30f);
        const float wgt = l > 0.f ? expf(m - M) : 0.f;
        const float L = wave_sum(wgt * l);
        sw[wr][lane] = wgt;
        if (lane == 0) sL[wr] = L;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NI; ++k) {
        const int j = t + 256 * k, r = j / (D / 4), c = (j % (D / 4)) * 4;
        if (j >= R * (D / 4)) continue;
        f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
        if (r0 + r < p.rows) {
            const float* py = p.part_y + ((size_t)(r0 + r) * ns * H + h) * D + c;
#pragma unroll
            for (int s = 0; s < NSP; ++s)
                if (s < ns) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) o[i] += sw[r][s] * yv[k][s][i];
                }
            for (int s = NSP; s < ns; ++s) {
                const f32x4 y = *reinterpret_cast<const f32x4*>(py + (size_t)s * H * D);
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] += sw[r][s] * y[i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] *= 1.0f / sL[r];
        }
        *reinterpret_cast<f32x4*>(&sy[r][c]) = o;
    }
    __syncthreads();
    float acc[R] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int it = 0; it < DMAX / 32; ++it) {
        if (it >= D / 32) continue;
        const int c = (it * 4 + q) * 8;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const f32x4 ya = *reinterpret_cast<const f32x4*>(&sy[r][c]), yb = *reinterpret_cast<const f32x4*>(&sy[r][c + 4]);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[r] = fmaf(ya[k], (float)wf[it][k], acc[r]);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[r] = fmaf(yb[k], (float)wf[it][4 + k], acc[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        acc[r] += __shfl_xor(acc[r], 1, 64);
        acc[r] += __shfl_xor(acc[r], 2, 64);
        if (q == 0 && r0 + r < p.rows) store_as(p.out, (size_t)(r0 + r) * D + h * 64 + e, acc[r] + p.bv[h * 64 + e], p.out_dtype);
    }
}

static int xattn_check(const XAttnParams& p) {
    if (p.H < 1 || p.H > 8 || p.d != 64 * p.H || p.rows <= 0 || p.nsplit < 1 || p.nsplit > 64 || p.n_keys < 1)
        return launch_refuse("xattn: needs 1 <= heads <= 8 of 64 dims, rows > 0, 1 <= nsplit <= 64");
    return WM_LAUNCH_OK;
}
int launch_xattn_absorb(const XAttnParams& p, hipStream_t st, bool late_loads) {
    if (const int rc = xattn_check(p)) return rc;
    static const bool late_env = wm_env("WM_ABSORB_LATE") != nullptr;  // developer build A/B: the loop that loads Wk after the barrier
    const dim3 grid((p.rows + 3) / 4, p.H), block(p.d / 2);
    if (late_loads || late_env)
        hipLaunchKernelGGL(xattn_absorb_kernel<false>, grid, block, 0, st, p);
    else
        hipLaunchKernelGGL(xattn_absorb_kernel<true>, grid, block, 0, st, p);
    return WM_LAUNCH_OK;
}
template <int H> static void launch_xattn_h(const XAttnParams& p, hipStream_t st, const int* utt_of) {
    // X is re-read by every layer of the step (147 MB for 128 rows: inside the 256 MB Infinity Cache).  WM_XATTN_NT (developer
    // build): non-temporal loads for A/B.
    static const bool nt = wm_env("WM_XATTN_NT") != nullptr;
    const dim3 grid(p.nsplit, p.rows), block(256);
    if (utt_of)  // n-best scoring: X by row map (rows of one clip re-read its X: never the non-temporal form)
        hipLaunchKernelGGL((xattn_map_kernel<H>), grid, block, 0, st, p, utt_of);
    else if (nt)
        hipLaunchKernelGGL((xattn_kernel<H, true>), grid, block, 0, st, p);
    else
        hipLaunchKernelGGL((xattn_kernel<H, false>), grid, block, 0, st, p);
}
int launch_xattn(const XAttnParams& p, hipStream_t st, const int* utt_of) {
    if (const int rc = xattn_check(p)) return rc;
    switch (p.H) {
        case 1: launch_xattn_h<1>(p, st, utt_of); break;
        case 2: launch_xattn_h<2>(p, st, utt_of); break;
        case 3: launch_xattn_h<3>(p, st, utt_of); break;
        case 4: launch_xattn_h<4>(p, st, utt_of); break;
        case 5: launch_xattn_h<5>(p, st, utt_of); break;
        case 6: launch_xattn_h<6>(p, st, utt_of); break;
        case 7: launch_xattn_h<7>(p, st, utt_of); break;
        default: launch_xattn_h<8>(p, st, utt_of); break;
    }
    return WM_LAUNCH_OK;
}
int launch_xattn_merge(const XAttnParams& p, hipStream_t st) {
    if (const int rc = xattn_check(p)) return rc;
    hipLaunchKernelGGL(xattn_merge_kernel, dim3((p.rows + 3) / 4, p.H), dim3(256), 0, st, p);
    return WM_LAUNCH_OK;
}

// ------------------------------------------------------------------------------------------------------------
// argmax with the reference's tie rule (strict '>' scanning upward => lowest index wins, whisper_tensor.mojo:436)
// + the greedy loop's bookkeeping (whisper.mojo:200-221): append the id, stop an utterance after its eot.
// block-wide (value, index) argmax of row[0..V): 16-byte loads (row 16-byte aligned, V rounded up inside the padded
// row), every load independent; ties resolve to the LOWEST index at every level.
__device__ __forceinline__ void argmax_block(const float* row, int V, float& best, int& bidx) {
    __shared__ float s_v[16];
    __shared__ int s_i[16];
    float mv = -INFINITY;
    int mi = 0x7fffffff;
    const int nv = V >> 2;
    for (int i = threadIdx.x; i < nv; i += blockDim.x) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * i);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (v[j] > mv) {  // increasing index within a thread: strict '>' keeps the lowest
                mv = v[j];
                mi = 4 * i + j;
            }
    }
    for (int i = (nv << 2) + threadIdx.x; i < V; i += blockDim.x) {
        const float v = row[i];
        if (v > mv || (v == mv && i < mi)) {
            mv = v;
            mi = i;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float v2 = __shfl_xor(mv, o, 64);
        const int i2 = __shfl_xor(mi, o, 64);
        if (v2 > mv || (v2 == mv && i2 < mi)) {
            mv = v2;
            mi = i2;
        }
    }
    const int wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_v[wid] = mv;
        s_i[wid] = mi;
    }
    __syncthreads();
    mv = s_v[0];
    mi = s_i[0];
    for (int k = 1; k < nw; ++k)
        if (s_v[k] > mv || (s_v[k] == mv && s_i[k] < mi)) {
            mv = s_v[k];
            mi = s_i[k];
        }
    best = mv;
    bidx = mi;
}
// stage 2 of the fused argmax: best of the per-workgroup partials of one utterance (ties -> lowest index)
__device__ __forceinline__ void argmax_partials(const float* pv, const int* pi, int n, float& best, int& bidx) {
    __shared__ float s_v[16];
    __shared__ int s_i[16];
    float mv = -INFINITY;
    int mi = 0x7fffffff;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const float v = pv[i];
        const int ix = pi[i];
        if (v > mv || (v == mv && ix < mi)) {
            mv = v;
            mi = ix;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float v2 = __shfl_xor(mv, o, 64);
        const int i2 = __shfl_xor(mi, o, 64);
        if (v2 > mv || (v2 == mv && i2 < mi)) {
            mv = v2;
            mi = i2;
        }
    }
    const int wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_v[wid] = mv;
        s_i[wid] = mi;
    }
    __syncthreads();
    mv = s_v[0];
    mi = s_i[0];
    for (int k = 1; k < nw; ++k)
        if (s_v[k] > mv || (s_v[k] == mv && s_i[k] < mi)) {
            mv = s_v[k];
            mi = s_i[k];
        }
    best = mv;
    bidx = mi;
}
// Repetition processors: the ids that would complete an n-gram the history holds.  hist(i), i < L, is the row's history;
// with n >= 2 and L >= n - 1, every position i with i + n - 1 < L whose n - 1 ids equal the last n - 1 names the id hist(i + n - 1).
// One compare chain per position, the positions spread over the workgroup; SET: the ids' bits are set in `ban`, else cleared —
// clearing walks the history the set was built from, so it costs what setting cost and no list of the set bits is kept.
template <bool SET, typename H>
__device__ __forceinline__ void repeat_ban_walk(unsigned* ban, int n, int L, H hist) {
    if (n < 2 || L < n - 1) return;
    const int s0 = L - (n - 1);
    for (int i = threadIdx.x; i + n - 1 < L; i += blockDim.x) {
        bool same = true;
        for (int k = 0; k < n - 1 && same; ++k) same = hist(i + k) == hist(s0 + k);
        if (same) {
            const int t = hist(i + n - 1);
            if (SET)
                atomicOr(ban + (t >> 5), 1u << (t & 31));
            else
                atomicAnd(ban + (t >> 5), ~(1u << (t & 31)));
        }
    }
}
// Sequence bias / bad words: a row's slots and bits for its NEXT step.  hist(i), i < L, is the row's history.  Pass 1, the
// sequences spread over the workgroup: sequence q of m ids matches when m = 1 (a length-1 ban of the eot is dropped), or when
// 2 <= m <= L and its first m - 1 ids are the history's last m - 1 (m <= L, not m - 1 <= L: HF's own `continue`) — a compare chain of at
// most 31 ids.  Pass 2, the slots spread over the workgroup: ONE thread walks its slot's sequences in table order and adds the matching
// biases, so the fp32 sum is HF's whichever thread matched what; it rewrites the SeqSlot and touches the id's bit only where the slot
// goes on or off, so nothing is swept.  FRESH: the bits were just cleared and no slot is on yet (the init kernel).
template <bool FRESH, typename H>
__device__ __forceinline__ void seq_bias_update(const SeqBiasCtl& c, unsigned* hit, SeqSlot* val, int L, H hist) {
    __shared__ unsigned char s_match[SEQ_BIAS_MAX];
    const int n_seq = min(c.n_seq, SEQ_BIAS_MAX), n_slots = min(c.n_slots, SEQ_BIAS_MAX);
    for (int q = threadIdx.x; q < n_seq; q += blockDim.x) {
        const int o = c.off[q], m = c.off[q + 1] - o;
        bool same;
        if (m == 1) {
            same = !(c.ban[q] && c.ids[o] == c.eot);
        } else {
            same = m <= L;
            for (int k = 0; k < m - 1 && same; ++k) same = hist(L - (m - 1) + k) == c.ids[o + k];
        }
        s_match[q] = same;
    }
    __syncthreads();
    for (int s = threadIdx.x; s < n_slots; s += blockDim.x) {
        float sum = 0.f;
        int flags = 0;
        for (int q = c.slot_off[s]; q < c.slot_off[s + 1]; ++q) {
            if (!s_match[q]) continue;
            flags |= 1;
            if (c.ban[q])
                flags |= 2;
            else
                sum += c.bias[q];
        }
        const int was = FRESH ? 0 : val[s].flags;
        val[s] = SeqSlot{sum, flags};
        if ((flags ^ was) & 1) {
            const int t = c.slot_id[s];
            if (flags & 1)
                atomicOr(hit + (t >> 5), 1u << (t & 31));
            else
                atomicAnd(hit + (t >> 5), ~(1u << (t & 31)));
        }
    }
}
// Phrase-list constraint: the trie node a row reaches from `node` along id t.  An id >= free_from is free and leaves the
// node where it is; otherwise the workgroup compares t with the node's edges (ids are distinct inside a node: at most one thread
// finds it) and the row moves to that child, or to the dead node, which has no edges and so keeps every later id.
__device__ __forceinline__ int constraint_advance(const ConstraintCtl& c, int node, int t) {
    __shared__ int s_next;
    if (t >= c.free_from) return node;  // (uniform over the workgroup: every thread holds the same t)
    if (threadIdx.x == 0) s_next = c.dead;
    __syncthreads();
    for (int e = c.edge_off[node] + (int)threadIdx.x; e < c.edge_off[node + 1]; e += blockDim.x)
        if (c.edge_id[e] == t) s_next = c.edge_next[e];
    __syncthreads();
    return s_next;
}
// The row's `ban` set for its NEXT step under the constraint: all `words` words rewritten.  First the complement of the node's allowed
// set — every id below min(free_from, V) banned, bits past V clear as the other sets keep them, then the bits of the node's edges and,
// where a phrase ends or the row has left the trie, of the eot cleared again — and behind a barrier the n-gram bans on top: the walk over the history for n >= 2,
// the ids of `seen` for n = 1 (`seen` already holds the history's last id).  hist(i), i < L, is the row's history.
template <typename H>
__device__ __forceinline__ void constraint_rewrite(const ConstraintCtl& c, unsigned* ban, const unsigned* seen, int words, int V, int node, int n,
                                                   int L, H hist) {
    const int lim = min(max(c.free_from, 0), V);
    for (int w = threadIdx.x; w < words; w += blockDim.x) {
        const int lo = w * 32;
        ban[w] = lo + 32 <= lim ? 0xffffffffu : lo >= lim ? 0u : (1u << (lim - lo)) - 1u;
    }
    __threadfence();
    __syncthreads();
    for (int e = c.edge_off[node] + (int)threadIdx.x; e < c.edge_off[node + 1]; e += blockDim.x) {
        const int t = c.edge_id[e];
        if ((unsigned)t < (unsigned)V) atomicAnd(ban + (t >> 5), ~(1u << (t & 31)));
    }
    // (the eot ends a phrase, and it is the dead node's way out: its allowed set is the eot and the free ids, never empty)
    if (threadIdx.x == 0 && (c.terminal[node] >= 0 || node == c.dead) && (unsigned)c.eot < (unsigned)V)
        atomicAnd(ban + (c.eot >> 5), ~(1u << (c.eot & 31)));
    __threadfence();
    __syncthreads();  // every allowed id is cleared before the first n-gram ban is set: an allowed id the n-gram bans stays banned
    if (n == 1) {
        for (int w = threadIdx.x; w < words; w += blockDim.x)
            if (const unsigned sw = seen[w]) atomicOr(ban + w, sw);  // (an atomic like every other update of the set behind its first store)
    } else {
        repeat_ban_walk<true>(ban, n, L, hist);
    }
}
// LP: the log-probability instantiation (p.lp_s non-null); LP = false is the kernel without it, static LDS included.  RP: the
// repetition processors' bookkeeping (p.rp_seen non-null), likewise.  SB: the sequence-bias bookkeeping (p.sb_hit non-null, needs RP).
// TK (top-k alternatives; p.tk_rows non-null, needs LP): thread 0 also leaves the row's TopkRow for the selection launch.
// CT (phrase-list constraint; p.ct_node non-null, needs RP): the row's trie node moves and its `ban` set is rewritten.
// The body of both kernels below: argmax_step_kernel is CT = false under the names it always had, argmax_step_ct_kernel CT = true.
template <bool LP, bool RP, bool SB, bool TK, bool CT, typename P>
__device__ __forceinline__ void argmax_step_body(const P p) {  // (by value, as the kernels took it: a reference costs the log-prob ones an SGPR)
    static_assert(LP || !TK, "the top-k alternatives ride the log-prob instantiation");
    static_assert(RP || !CT, "the constraint writes the repetition processors' ban set");
    const int b = blockIdx.x;
    if (p.ts && b == 0 && threadIdx.x == 0) ts_put(p.ts, p.ts_id, 3);
    const int pos0 = p.emb_out ? p.pos[b] : 0;  // read before thread 0 advances it (the reductions below synchronise)
    int rp_len = -1;  // RP: the row's history length before this id, -1 = the row stores nothing (read before thread 0 appends)
    if constexpr (RP) rp_len = p.finished[b] ? -1 : p.n_tokens[b];
    if (p.host_progress && b == 0 && threadIdx.x == 0) {
        // finishes of EARLIER steps are complete (their launches ended); this step's may or may not be counted yet: a lower bound.
        // System-scope stores to pinned host memory: visible to the polling host without any stream synchronisation.
        const int fin = __hip_atomic_load(&p.ctl->n_finished, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&p.host_progress[0], fin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&p.host_progress[1], p.ctl->len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    float best;
    int idx;
    if (p.pval)
        argmax_partials(p.pval + (size_t)b * p.npart, p.pidx + (size_t)b * p.npart, p.npart, best, idx);
    else
        argmax_block(p.logits + (size_t)b * p.ldl, p.V, best, idx);
    // Log-probabilities (lp_s null = off): lp = s[id] - logsumexp(s) over what the processors leave.  Text side: part k
    // contributes lp_s[k] * exp(pval[k] - best) — the exp terms by all threads, the sum by thread 0 in ascending part order, so a
    // row's value does not depend on the batch it sits in.
    float txt_s = 0.f, lp = -INFINITY;  // thread 0: sum of exp(text - best); the chosen id's log-probability
    if constexpr (LP) {
        __shared__ float s_term[256];
        for (int k0 = 0; k0 < p.npart; k0 += 256) {
            const int k = k0 + (int)threadIdx.x;
            if (threadIdx.x < 256 && k < p.npart) {
                const float s2 = p.lp_s[(size_t)b * p.npart + k];
                s_term[threadIdx.x] = s2 > 0.f ? s2 * expf(p.pval[(size_t)b * p.npart + k] - best) : 0.f;
            }
            __syncthreads();
            if (threadIdx.x == 0)
                for (int j = 0; j < min(256, p.npart - k0); ++j) txt_s += s_term[j];
            __syncthreads();
        }
        if (!p.ts_state && txt_s > 0.f) lp = -logf(txt_s);  // best - (best + log sum); every candidate -inf: stays -inf, never NaN
    }
    TopkRow tk{};  // TK, thread 0: rules off — everything the mask leaves, against (best, log of the text sum)
    if constexpr (TK) {
        tk.hi0 = p.V;
        tk.ref = best;
        tk.logz = txt_s > 0.f ? logf(txt_s) : 0.f;
    }
    if (p.ts_state) {
        // Timestamp rules, the decision (HF WhisperTimeStampLogitsProcessor rule 5 + the final argmax): (best, idx) is the best
        // admissible text id; if the admissible timestamps' probability mass exceeds it — logsumexp(ts) > best, the softmax
        // normaliser being common — the id is the best admissible timestamp.  (Without that the argmax over both sets would
        // still be a text id: logsumexp(ts) >= max(ts).)  Then the history and the NEXT argmax's ranges.
        __shared__ int s_pick;
        if (threadIdx.x == 0) {
            float tv = -INFINITY, tm = -INFINITY, tsum = 0.f;
            int ti = 0x7fffffff;
            for (int k = p.ts_part0; k < p.npart; ++k) {  // <= a dozen parts, fixed order
                const size_t o = (size_t)b * p.npart + k;
                const float v2 = p.ts_val[o], m2 = p.ts_m[o], s2 = p.ts_s[o];
                const int i2 = p.ts_idx[o];
                if (v2 > tv || (v2 == tv && i2 < ti)) {
                    tv = v2;
                    ti = i2;
                }
                const float mn = fmaxf(tm, m2);
                tsum = (tsum > 0.f ? tsum * expf(tm - mn) : 0.f) + (s2 > 0.f ? s2 * expf(m2 - mn) : 0.f);
                tm = mn;
            }
            int pick = idx;
            const bool have_text = (unsigned)idx < (unsigned)p.V;
            const bool forced = tsum > 0.f && (!have_text || tm + logf(tsum) > best);
            if (forced) pick = ti;
            if constexpr (LP) {
                // forced timestamp: HF sets every text id to -inf, the normaliser is the admissible timestamps' alone; else text ∪ timestamps
                if (forced) {
                    lp = (tv - tm) - logf(tsum);  // differences first: a row offset by 1e4 keeps its low bits
                } else if (have_text) {
                    const float mn = fmaxf(best, tm);
                    const float tot = (txt_s > 0.f ? txt_s * expf(best - mn) : 0.f) + (tsum > 0.f ? tsum * expf(tm - mn) : 0.f);
                    if (tot > 0.f) lp = (best - mn) - logf(tot);
                }
            }
            if constexpr (TK) {  // this step's ranges, before the history moves on; the pair the branch above normalised with
                const TsState cur = p.ts_state[b];
                tk.lo1 = cur.ts_lo;
                tk.hi1 = cur.ts_hi;
                if (forced) {
                    tk.lo0 = tk.hi0 = 0;
                    tk.ref = tm;
                    tk.logz = logf(tsum);
                } else {
                    const float mn = fmaxf(best, tm);
                    const float tot = (txt_s > 0.f ? txt_s * expf(best - mn) : 0.f) + (tsum > 0.f ? tsum * expf(tm - mn) : 0.f);
                    tk.lo0 = cur.text_lo;
                    tk.hi0 = cur.text_hi;
                    tk.ref = mn;
                    tk.logz = tot > 0.f ? logf(tot) : 0.f;
                }
            }
            if ((unsigned)pick >= (unsigned)p.V) pick = 0;
            TsState st = p.ts_state[b];
            const int is_ts = pick >= p.rules.tb;
            st.pen_ts = st.n_gen + 1 < 2 ? 1 : st.last_ts;
            st.last_ts = is_ts;
            st.n_gen += 1;
            if (is_ts) st.t_last = pick;
            ts_next_ranges(st, p.rules);
            p.ts_state[b] = st;
            s_pick = pick;
        }
        __syncthreads();
        idx = s_pick;
    }
    // every candidate NaN / -inf (16-bit overflow, bad weights, a mask over the whole vocabulary): no comparison succeeded and
    // idx is still the sentinel — it must not become an embedding row index.  The reference's scan (whisper_tensor.mojo:431-439:
    // start at t[0], strict '>') returns index 0 in exactly these cases, and so does this.
    if ((unsigned)idx >= (unsigned)p.V) idx = 0;
    if (threadIdx.x == 0) {
        p.next[b] = idx;
        if (LP && p.lp_next) p.lp_next[b] = lp;
        if constexpr (TK) {  // the entry beside the id's: same guard as out_tokens (read before this step's count and finish)
            tk.slot = !p.out_tokens ? b : p.finished[b] ? -1 : b * p.out_stride + p.n_tokens[b];
            tk.id0 = idx;
            tk.lp0 = lp;
            p.tk_rows[b] = tk;
        }
        if (p.advance) {  // current_len += 1 (layers.mojo:143), position += 1: nothing else in this launch reads them
            p.pos[b] += 1;
            if (b == 0) p.ctl->len += 1;
        }
        if (p.out_tokens && !p.finished[b]) {
            p.out_tokens[(size_t)b * p.out_stride + p.n_tokens[b]] = idx;
            if (LP && p.logprobs) {
                p.logprobs[(size_t)b * p.out_stride + p.n_tokens[b]] = lp;
                p.lp_sum[b] += lp;
            }
            p.n_tokens[b] += 1;
            if (!p.ignore_eot && idx == p.eot) {
                p.finished[b] = 1;
                atomicAdd(&p.ctl->n_finished, 1);
            }
        }
    }
    if constexpr (RP) {
        // a row that stored its id: the history is out_tokens[b][0 .. rp_len) and the new id (every thread holds it; thread 0's store
        // of it is not read here).  `ban` loses the bits of this step — the walk over the history without the new id that set them —
        // and gains those of the next one.  n = 1 bans every id of the history: `ban` follows `seen` and nothing is ever cleared.
        if (rp_len >= 0) {
            const int n = p.rp_ctl->ngram;
            unsigned* seen = p.rp_seen + (size_t)b * p.rp_words;
            unsigned* ban = p.rp_ban + (size_t)b * p.rp_words;
            const int* row = p.out_tokens + (size_t)b * p.out_stride;
            const int L = rp_len;
            auto hist = [&](int i) { return i < L ? row[i] : idx; };
            if constexpr (CT) {
                // the constrained row: its node moves along the new id, and the whole set is written again for the new node — the
                // constraint's words first, the n-gram bans of the next step on top — so nothing of this step has to be cleared
                const ConstraintCtl c = *p.ct_ctl;
                if (threadIdx.x == 0) atomicOr(seen + (idx >> 5), 1u << (idx & 31));
                const int node = p.ct_node[b];
                const int to = constraint_advance(c, node, idx);
                if (threadIdx.x == 0) {
                    if (!p.ignore_eot && idx == p.eot) p.ct_match[b] = c.terminal[node];  // the row ends here: the phrase it stood on
                    p.ct_node[b] = to;
                }
                constraint_rewrite(c, ban, seen, p.rp_words, p.V, to, n, L + 1, hist);
            } else {
                if (threadIdx.x == 0) {
                    atomicOr(seen + (idx >> 5), 1u << (idx & 31));
                    if (n == 1) atomicOr(ban + (idx >> 5), 1u << (idx & 31));
                }
                repeat_ban_walk<false>(ban, n, L, hist);
                __threadfence();
                __syncthreads();  // every clear is done before the first set: an id banned at both steps stays banned
                repeat_ban_walk<true>(ban, n, L + 1, hist);
            }
            if constexpr (SB)
                seq_bias_update<false>(*p.sb_ctl, p.sb_hit + (size_t)b * p.rp_words, p.sb_val + (size_t)b * SEQ_BIAS_MAX, L + 1, hist);
        }
    }
    if (p.emb_out) {  // every thread holds idx: next step's embedding row (whisper.mojo:141-149)
        const float* te = p.emb_tok + (size_t)idx * p.d;
        const float* pe = p.emb_pos + (size_t)min(pos0 + (p.advance ? 1 : 0), p.max_pos) * p.d;
        for (int j = threadIdx.x; j < p.d; j += blockDim.x) p.emb_out[(size_t)b * p.d + j] = te[j] + pe[j];
    }
}
template <bool LP, bool RP = false, bool SB = false, bool TK = false>
__global__ __launch_bounds__(1024) void argmax_step_kernel(ArgmaxParams p) {
    argmax_step_body<LP, RP, SB, TK, false>(p);
}
template <bool LP, bool SB, bool TK>
__global__ __launch_bounds__(256) void argmax_step_ct_kernel(ArgmaxCtParams p) {
    argmax_step_body<LP, true, SB, TK, true>(p);
}
template <bool LP, bool SB, bool TK> static void launch_argmax_constrained(const ArgmaxCtParams& p, hipStream_t st) {
    hipLaunchKernelGGL((argmax_step_ct_kernel<LP, SB, TK>), dim3(p.B), dim3(256), 0, st, p);
}
// the constraint's instantiations: the repetition processors' ones (with or without the rest) plus the trie walk
int launch_argmax_step_ct(const ArgmaxCtParams& p, hipStream_t st) {
    if (!p.ct_node || !p.ct_match || !p.ct_ctl) return launch_refuse("argmax_step: the constraint needs the rows' nodes, their matches and the control block");
    if (!p.rp_seen || !p.out_tokens || !p.pval || !p.rp_ban || !p.rp_ctl || p.rp_words < repeat_words(p.V))
        return launch_refuse("argmax_step: the constraint needs the repetition processors' partials form, the id table, both sets and their control block");
    if (p.sb_hit && (!p.sb_val || !p.sb_ctl)) return launch_refuse("argmax_step: the sequence bias needs the rows' slots and the control block");
    if (p.tk_rows && !p.lp_s) return launch_refuse("argmax_step: the top-k alternatives need the log-prob form");
    if (p.tk_rows)
        p.sb_hit ? launch_argmax_constrained<true, true, true>(p, st) : launch_argmax_constrained<true, false, true>(p, st);
    else if (p.lp_s)
        p.sb_hit ? launch_argmax_constrained<true, true, false>(p, st) : launch_argmax_constrained<true, false, false>(p, st);
    else
        p.sb_hit ? launch_argmax_constrained<false, true, false>(p, st) : launch_argmax_constrained<false, false, false>(p, st);
    return WM_LAUNCH_OK;
}
int launch_argmax_step(const ArgmaxParams& p, hipStream_t st) {
    if (p.tk_rows) {  // the top-k instantiations: the log-prob ones plus the row's TopkRow, nothing else differs
        if (!p.lp_s || !p.pval) return launch_refuse("argmax_step: the top-k alternatives need the log-prob form");
        if (p.sb_hit && (!p.rp_seen || !p.sb_val || !p.sb_ctl)) return launch_refuse("argmax_step: the sequence bias needs the repetition processors' sets, the rows' slots and the control block");
        if (p.rp_seen && (!p.out_tokens || !p.rp_ban || !p.rp_ctl || p.rp_words < repeat_words(p.V)))
            return launch_refuse("argmax_step: the repetition processors need the partials form, the id table, both sets and their control block");
        if (p.sb_hit)
            hipLaunchKernelGGL((argmax_step_kernel<true, true, true, true>), dim3(p.B), dim3(256), 0, st, p);
        else if (p.rp_seen)
            hipLaunchKernelGGL((argmax_step_kernel<true, true, false, true>), dim3(p.B), dim3(256), 0, st, p);
        else
            hipLaunchKernelGGL((argmax_step_kernel<true, false, false, true>), dim3(p.B), dim3(256), 0, st, p);
        return WM_LAUNCH_OK;
    }
    if (p.rp_seen) {  // the sets' bookkeeping reads the row's history and rides the partials form: anything else is refused, not dropped
        if (!p.out_tokens || !p.pval || !p.rp_ban || !p.rp_ctl || p.rp_words < repeat_words(p.V))
            return launch_refuse("argmax_step: the repetition processors need the partials form, the id table, both sets and their control block");
        if (p.sb_hit) {
            if (!p.sb_val || !p.sb_ctl) return launch_refuse("argmax_step: the sequence bias needs the rows' slots and the control block");
            if (p.lp_s)
                hipLaunchKernelGGL((argmax_step_kernel<true, true, true>), dim3(p.B), dim3(256), 0, st, p);
            else
                hipLaunchKernelGGL((argmax_step_kernel<false, true, true>), dim3(p.B), dim3(256), 0, st, p);
            return WM_LAUNCH_OK;
        }
        if (p.lp_s)
            hipLaunchKernelGGL((argmax_step_kernel<true, true>), dim3(p.B), dim3(256), 0, st, p);
        else
            hipLaunchKernelGGL((argmax_step_kernel<false, true>), dim3(p.B), dim3(256), 0, st, p);
        return WM_LAUNCH_OK;
    }
    if (p.sb_hit) return launch_refuse("argmax_step: the sequence bias needs the repetition processors' sets");
    if (p.lp_s && p.pval)
        hipLaunchKernelGGL(argmax_step_kernel<true>, dim3(p.B), dim3(256), 0, st, p);
    else
        hipLaunchKernelGGL(argmax_step_kernel<false>, dim3(p.B), dim3(p.pval ? 256 : 1024), 0, st, p);
    return WM_LAUNCH_OK;
}
// Top-k alternatives, the selection: one workgroup of 4 waves per row.  A thread keeps the TOPK_MAX best of the ids
// threadIdx.x, + 256, ... (ascending, so strict '>' keeps the lowest id among equals) as a sorted list in registers; a wave pops its
// lanes' heads TOPK_MAX times (a butterfly arg-max per pop: value, then lowest id), thread 0 merges the 4 waves' lists from LDS the
// same way.  Every order is fixed by values and ids alone: a row's result does not depend on the batch it sits in.
__device__ __forceinline__ bool topk_before(float v, int i, float v2, int i2) { return v > v2 || (v == v2 && i < i2); }
__global__ __launch_bounds__(256) void topk_select_kernel(TopkSelectParams p) {
    constexpr int K = TOPK_MAX;
    const int b = blockIdx.x;
    const TopkRow row = p.rows[b];
    if (row.slot < 0) return;  // (block-uniform) a finished row stores nothing
    __shared__ float s_v[4][K];
    __shared__ int s_i[4][K];
    const float* z = p.logits + (size_t)b * p.ldl;
    float lv[K];
    int li[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        lv[j] = -INFINITY;
        li[j] = 0x7fffffff;
    }
    for (int n = threadIdx.x; n < p.V; n += 256) {
        if (!((n >= row.lo0 && n < row.hi0) || (n >= row.lo1 && n < row.hi1))) continue;
        const float v = z[n] + (p.mask ? p.mask[n] : 0.f);
        if (v > lv[K - 1] && v < INFINITY) {  // (NaN and -inf fail the compare; n only grows: an equal value never displaces)
            lv[K - 1] = v;
            li[K - 1] = n;
#pragma unroll
            for (int j = K - 1; j > 0; --j)
                if (lv[j] > lv[j - 1]) {
                    const float tv = lv[j];
                    const int ti = li[j];
                    lv[j] = lv[j - 1];
                    li[j] = li[j - 1];
                    lv[j - 1] = tv;
                    li[j - 1] = ti;
                }
        }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int r = 0; r < K; ++r) {
        float bv = lv[0];
        int bi = li[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float v2 = __shfl_xor(bv, o, 64);
            const int i2 = __shfl_xor(bi, o, 64);
            if (topk_before(v2, i2, bv, bi)) {
                bv = v2;
                bi = i2;
            }
        }
        if (bv > -INFINITY && bi == li[0]) {  // ids are unique: exactly the lane that held the winner pops it
#pragma unroll
            for (int j = 0; j < K - 1; ++j) {
                lv[j] = lv[j + 1];
                li[j] = li[j + 1];
            }
            lv[K - 1] = -INFINITY;
            li[K - 1] = 0x7fffffff;
        }
        if (lane == 0) {
            s_v[w][r] = bv;
            s_i[w][r] = bv > -INFINITY ? bi : 0x7fffffff;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int head[4] = {0, 0, 0, 0};
        int* oi = p.ids + (size_t)row.slot * p.k;
        float* ol = p.lps + (size_t)row.slot * p.k;
        // rank 0: the id the step emitted, with the log-prob it stored (id 0 / -inf when nothing was finite).  The merged stream then
        // fills ranks 1.. and passes over the emitted id BY ID wherever it stands: an id is neither listed twice nor lost when the
        // arg-max's winner is not the stream's head (a +inf score, which the sweep leaves out)
        oi[0] = row.id0;
        ol[0] = row.lp0;
        for (int r = 1; r < p.k;) {
            float bv = -INFINITY;
            int bi = 0x7fffffff, bw = -1;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (head[q] >= K) continue;
                const float v2 = s_v[q][head[q]];
                const int i2 = s_i[q][head[q]];
                if (topk_before(v2, i2, bv, bi)) {
                    bv = v2;
                    bi = i2;
                    bw = q;
                }
            }
            if (bw >= 0) {
                head[bw] += 1;  // (every turn moves a head or r: at most 4 K + k turns)
                if (bi == row.id0) continue;
                oi[r] = bi;
                ol[r] = (bv - row.ref) - row.logz;
            } else {
                oi[r] = -1;
                ol[r] = -INFINITY;
            }
            ++r;
        }
    }
}
int launch_topk_select(const TopkSelectParams& p, hipStream_t st) {
    if (!p.logits || !p.rows || !p.ids || !p.lps || p.B <= 0 || p.V <= 0 || p.ldl < p.V) return launch_refuse("topk_select: bad argument");
    if (p.k < 1 || p.k > TOPK_MAX) return launch_refuse("topk_select: k must be 1..8");
    hipLaunchKernelGGL(topk_select_kernel, dim3(p.B), dim3(256), 0, st, p);
    return WM_LAUNCH_OK;
}
__global__ __launch_bounds__(1024) void argmax_plain_kernel(const float* t, int n, int* idx) {
    float best;
    int i;
    argmax_block(t, n, best, i);
    if ((unsigned)i >= (unsigned)n) i = 0;  // all-NaN / all -inf input: the reference's scan (whisper_tensor.mojo:431-439) returns 0
    if (threadIdx.x == 0) *idx = i;
}
void launch_argmax_plain(const float* t, int n, int* idx, hipStream_t st) {
    hipLaunchKernelGGL(argmax_plain_kernel, dim3(1), dim3(1024), 0, st, t, n, idx);
}

// start of a greedy run: tokens = prompt (whisper.mojo:187-191, 200-202), nothing finished, control block zeroed
__global__ void init_tokens_kernel(InitTokensParams p) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < p.B) {
        for (int i = 0; i < p.n_prompt; ++i) p.out_tokens[(size_t)b * p.out_stride + i] = p.prompt[i];
        p.n_tokens[b] = p.n_prompt;
        p.finished[b] = 0;
        if (p.logprobs) {  // prompt and tail positions of the log-prob table stay 0
            for (int i = 0; i < p.out_stride; ++i) p.logprobs[(size_t)b * p.out_stride + i] = 0.f;
            p.lp_sum[b] = 0.f;
        }
        if (p.tok_rows) {
            for (int i = 0; i < p.n_prompt; ++i) {
                p.tok_rows[i * p.B + b] = p.prompt[i];
                p.pos_rows[i * p.B + b] = i;
            }
        }
        if (p.ts_state) {
            TsState st;
            st.n_gen = 0;
            st.last_ts = 0;
            st.pen_ts = 1;
            st.t_last = -1;
            ts_next_ranges(st, p.rules);
            p.ts_state[b] = st;
        }
    }
    if (b == 0) {
        p.ctl->len = 0;
        p.ctl->n_finished = 0;
    }
}
void launch_init_tokens(const InitTokensParams& p, hipStream_t st) {
    hipLaunchKernelGGL(init_tokens_kernel, dim3((p.B + 255) / 256), dim3(256), 0, st, p);
}
// per-row prompts: row b's prompt is table[b][0 .. len[b]) (p.prompt / p.n_prompt unused).  The rows of the pass end together at
// position Lmax: row b has pad = Lmax - len[b] dead slots in front — (the row's first id, position 0) in the prefill rows, never attended to
// (key_lo[b] = pad).  out_tokens gets the row's own prompt, unpadded.
__global__ void init_tokens_rows_kernel(InitTokensParams p, RowPromptParams r) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < p.B) {
        const int Lb = r.len[b], pad = r.Lmax - Lb;
        const int* row = r.table + (size_t)b * r.stride;
        for (int i = 0; i < Lb; ++i) p.out_tokens[(size_t)b * p.out_stride + i] = row[i];
        p.n_tokens[b] = Lb;
        p.finished[b] = 0;
        if (p.logprobs) {
            for (int i = 0; i < p.out_stride; ++i) p.logprobs[(size_t)b * p.out_stride + i] = 0.f;
            p.lp_sum[b] = 0.f;
        }
        r.key_lo[b] = pad;
        for (int t = 0; t < r.Lmax; ++t) {
            p.tok_rows[(size_t)t * p.B + b] = t < pad ? row[0] : row[t - pad];
            p.pos_rows[(size_t)t * p.B + b] = t < pad ? 0 : t - pad;
        }
        if (p.ts_state) {
            TsState st;
            st.n_gen = 0;
            st.last_ts = 0;
            st.pen_ts = 1;
            st.t_last = -1;
            ts_next_ranges(st, p.rules);
            p.ts_state[b] = st;
        }
    }
    if (b == 0) {
        p.ctl->len = 0;
        p.ctl->n_finished = 0;
    }
}
void launch_init_tokens_rows(const InitTokensParams& p, const RowPromptParams& r, hipStream_t st) {
    hipLaunchKernelGGL(init_tokens_rows_kernel, dim3((p.B + 255) / 256), dim3(256), 0, st, p, r);
}
// start of a pass with the repetition processors, one workgroup per row, behind the init-tokens launch: both sets
// cleared, `seen` = the row's prompt, `ban` = what the prompt bans for the first generated id
__global__ __launch_bounds__(256) void repeat_init_kernel(RepeatInitParams p) {
    const int b = blockIdx.x;
    if (b == 0 && threadIdx.x == 0) *p.ctl = RepeatCtl{p.penalty, p.ngram};
    unsigned* seen = p.seen + (size_t)b * p.words;
    unsigned* ban = p.ban + (size_t)b * p.words;
    for (int i = threadIdx.x; i < p.words; i += blockDim.x) seen[i] = ban[i] = 0u;
    __threadfence();
    __syncthreads();
    const int* row = p.out_tokens + (size_t)b * p.out_stride;
    const int L = p.n_tokens[b];
    for (int i = threadIdx.x; i < L; i += blockDim.x) {
        const int t = row[i];
        atomicOr(seen + (t >> 5), 1u << (t & 31));
        if (p.ngram == 1) atomicOr(ban + (t >> 5), 1u << (t & 31));
    }
    repeat_ban_walk<true>(ban, p.ngram, L, [&](int i) { return row[i]; });
}
void launch_repeat_init(const RepeatInitParams& p, hipStream_t st) {
    hipLaunchKernelGGL(repeat_init_kernel, dim3(p.B), dim3(256), 0, st, p);
}
// start of a pass with sequence bias / bad words, one workgroup per row, behind the init-tokens launch: the control
// block, the row's bits cleared, its slots and bits for the first generated id from its prompt
__global__ __launch_bounds__(256) void seq_bias_init_kernel(SeqBiasInitParams p) {
    const int b = blockIdx.x;
    // A state with several decode lanes launches this once per lane, each on its own stream, and every launch writes the state's one
    // control block: the same table and eot, so the same bytes, and no kernel of the pass reads it before its own lane's init.
    if (b == 0 && threadIdx.x == 0) *p.ctl = p.table;
    unsigned* hit = p.hit + (size_t)b * p.words;
    for (int i = threadIdx.x; i < p.words; i += blockDim.x) hit[i] = 0u;
    __threadfence();
    __syncthreads();
    const int* row = p.out_tokens + (size_t)b * p.out_stride;
    seq_bias_update<true>(p.table, hit, p.val + (size_t)b * SEQ_BIAS_MAX, p.n_tokens[b], [&](int i) { return row[i]; });
}
int launch_seq_bias_init(const SeqBiasInitParams& p, hipStream_t st) {
    const SeqBiasCtl& t = p.table;
    if (!p.hit || !p.val || !p.ctl || !p.out_tokens || !p.n_tokens || p.B <= 0 || p.words <= 0 || t.n_seq < 1 || t.n_seq > SEQ_BIAS_MAX ||
        t.n_slots < 1 || t.n_slots > t.n_seq || !t.ids || !t.off || !t.bias || !t.ban || !t.slot_id || !t.slot_off || !t.slot_of)
        return launch_refuse("seq_bias_init: 1 .. SEQ_BIAS_MAX sequences in at most as many slots, and every table");
    hipLaunchKernelGGL(seq_bias_init_kernel, dim3(p.B), dim3(256), 0, st, p);
    return WM_LAUNCH_OK;
}
// start of a pass with a phrase-list constraint, one workgroup per row, behind the repeat-init launch that cleared the
// sets and filled `seen` from the prompt: the control block, the row on the root with no match, and the root's allowed set,
// complemented, over the row's `ban` with the prompt's n-gram bans set again on top
__global__ __launch_bounds__(256) void constraint_init_kernel(ConstraintInitParams p) {
    const int b = blockIdx.x;
    // (several decode lanes: every lane's launch writes the state's one control block with the same bytes, as seq_bias_init_kernel does)
    if (b == 0 && threadIdx.x == 0) *p.ctl = p.table;
    if (threadIdx.x == 0) {
        p.node[b] = 0;
        p.match[b] = -1;
    }
    const int* row = p.out_tokens + (size_t)b * p.out_stride;
    constraint_rewrite(p.table, p.ban + (size_t)b * p.words, p.seen + (size_t)b * p.words, p.words, p.vocab, 0, p.ngram, p.n_tokens[b],
                       [&](int i) { return row[i]; });
}
int launch_constraint_init(const ConstraintInitParams& p, hipStream_t st) {
    const ConstraintCtl& t = p.table;
    if (!p.ban || !p.seen || !p.node || !p.match || !p.ctl || !p.out_tokens || !p.n_tokens || p.B <= 0 || p.vocab <= 0 ||
        p.words < repeat_words(p.vocab) || t.n_nodes < 2 || t.n_nodes > CONSTRAINT_NODES_MAX || t.dead < 1 || t.dead >= t.n_nodes || !t.edge_off ||
        !t.edge_id || !t.edge_next || !t.terminal)
        return launch_refuse("constraint_init: 2 .. CONSTRAINT_NODES_MAX nodes with a dead node among them, every table and ceil(vocab / 32) words per row");
    hipLaunchKernelGGL(constraint_init_kernel, dim3(p.B), dim3(256), 0, st, p);
    return WM_LAUNCH_OK;
}
// end of a per-row prefill: cache length Lmax for all, position len[b] + pos_delta per row
__global__ void set_rows_step_kernel(StepCtl* ctl, int Lmax, int* pos, const int* len, int pos_delta, int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) pos[i] = len[i] + pos_delta;
    if (i == 0) ctl->len = Lmax;
}
void launch_set_rows_step(StepCtl* ctl, int Lmax, int* pos, const int* len, int pos_delta, int B, hipStream_t st) {
    hipLaunchKernelGGL(set_rows_step_kernel, dim3((B + 255) / 256), dim3(256), 0, st, ctl, Lmax, pos, len, pos_delta, B);
}

__global__ void pack_tokens_kernel(const int* __restrict__ out_tokens, const int* __restrict__ n_tokens, int out_stride, int rows, int stride,
                                   int* __restrict__ dst) {
    const int r = blockIdx.x;
    int* d = dst + (size_t)r * (1 + stride);
    const int n = r < rows ? min(n_tokens[r], stride) : 0;
    if (threadIdx.x == 0) d[0] = n;
    for (int j = threadIdx.x; j < stride; j += blockDim.x) d[1 + j] = j < n ? out_tokens[(size_t)r * out_stride + j] : 0;
}
void launch_pack_tokens(const int* out_tokens, const int* n_tokens, int out_stride, int rows, int rows_cap, int stride, int* dst, hipStream_t st) {
    hipLaunchKernelGGL(pack_tokens_kernel, dim3(rows_cap), dim3(256), 0, st, out_tokens, n_tokens, out_stride, rows, stride, dst);
}

__global__ void set_step_kernel(StepCtl* ctl, int len, int set_len, int* pos, int pos_value, int* tok, int tok_value, int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) {
        if (pos) pos[i] = pos_value;
        if (tok) tok[i] = tok_value;
    }
    if (i == 0 && set_len) ctl->len = len;
}
void launch_set_step(StepCtl* ctl, int len, int set_len, int* pos, int pos_value, int* tok, int tok_value, int B,
                     hipStream_t st) {
    hipLaunchKernelGGL(set_step_kernel, dim3((B + 255) / 256), dim3(256), 0, st, ctl, len, set_len, pos, pos_value, tok,
                       tok_value, B);
}

// ------------------------------------------------------------------------------------------------------------
// No-speech probe: HF WhisperNoSpeechDetection — softmax over the RAW logits at the <|startoftranscript|> position,
// read at no_speech_token.  The prefill keeps each row's last-layer residual row of that position (capture); after the prefill the
// LP instantiation of the logits kernel sweeps the vocabulary once over those rows with no mask and no ranges, into the probe's own
// partials: per part (max, Σ exp(v − max)); the finish kernel merges them and reads the token's probability.
__global__ void no_speech_capture_kernel(const float* __restrict__ rows, float* __restrict__ out, int n4) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n4) reinterpret_cast<f32x4*>(out)[i] = reinterpret_cast<const f32x4*>(rows)[i];
}
void launch_no_speech_capture(const float* rows, float* out, int B, int d, hipStream_t st) {
    const int n4 = B * d / 4;  // d is a multiple of 128
    hipLaunchKernelGGL(no_speech_capture_kernel, dim3((n4 + 255) / 256), dim3(256), 0, st, rows, out, n4);
}
// One workgroup per row.  M = the parts' largest maximum (exact in any order); thread k forms psum[k]·exp(pmax[k] − M), thread 0 adds
// the terms in ascending part order (a fixed order: a row's value does not depend on the batch it rides in).  Wave 0 recomputes the
// token's logit as the logits kernel forms it: fp32 LayerNorm of the row (one-pass statistics, eps 1e-5), rounded to the operand
// dtype TW, times the token's embedding row, summed in fp32.  log p = (logit − M) − log S: the maxima are subtracted first, so every
// exponent is <= 0 and an offset of the whole row costs nothing.
template <typename TW>
__global__ __launch_bounds__(256) void no_speech_finish_kernel(NoSpeechParams p) {
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    __shared__ float s_red[4];
    __shared__ float s_term[256];
    __shared__ float s_logit;
    const float* pm = p.pmax + (size_t)b * p.stride;
    const float* ps = p.psum + (size_t)b * p.stride;
    float mx = -INFINITY;
    for (int k = tid; k < p.npart; k += 256) mx = fmaxf(mx, pm[k]);
    mx = wave_max(mx);
    if (lane == 0) s_red[w] = mx;
    if (w == 0) {
        const float* xr = p.x + (size_t)b * p.ldx;
        float sm = 0.f, sq = 0.f;
        for (int k = lane; k < p.K; k += 64) {
            const float v = xr[k];
            sm += v;
            sq += v * v;
        }
        sm = wave_sum(sm);
        sq = wave_sum(sq);
        const float mean = sm / (float)p.K;
        const float var = (sq / (float)p.K) - (mean * mean);
        const float rstd = 1.0f / sqrtf(fmaxf(var, 0.f) + 1e-5f);
        const TW* er = (const TW*)p.emb + (size_t)p.token * p.K;
        float acc = 0.f;
        for (int k = lane; k < p.K; k += 64) {
            const TW a = from_f32<TW>((xr[k] - mean) * rstd * p.ln_g[k] + p.ln_b[k]);
            acc += (float)a * (float)er[k];
        }
        acc = wave_sum(acc);
        if (lane == 0) s_logit = acc;
    }
    __syncthreads();
    const float M = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
    float S = 0.f;
    for (int k0 = 0; k0 < p.npart; k0 += 256) {
        const int k = k0 + tid;
        float t = 0.f;
        if (k < p.npart) {
            const float s2 = ps[k];
            if (s2 > 0.f) t = s2 * expf(pm[k] - M);
        }
        s_term[tid] = t;
        __syncthreads();
        if (tid == 0) {
            const int n = min(256, p.npart - k0);
            for (int j = 0; j < n; ++j) S += s_term[j];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const float ls = logf(S);  // S >= 1: the part that holds M contributes a term exp(0)
        p.lse[b] = M + ls;
        p.prob[b] = expf(fminf((s_logit - M) - ls, 0.f));
    }
}
template <typename TW> void launch_no_speech_finish(const NoSpeechParams& p, hipStream_t st) {
    hipLaunchKernelGGL(no_speech_finish_kernel<TW>, dim3(p.B), dim3(256), 0, st, p);
}
template void launch_no_speech_finish<float>(const NoSpeechParams&, hipStream_t);
template void launch_no_speech_finish<bf16>(const NoSpeechParams&, hipStream_t);
template void launch_no_speech_finish<f16>(const NoSpeechParams&, hipStream_t);

// ------------------------------------------------------------------------------------------------------------
// Language detection: HF WhisperGenerationMixin.detect_language — the logits of a decoder pass over
// [<|startoftranscript|>] alone, everything outside the language ids at -inf, arg-max; openai-whisper also returns the softmax over
// the languages.  Only the n_lang candidate columns are formed (n_lang·K embedding elements, not the vocabulary's N·K).
// One workgroup per row.  The LayerNorm is the one of no_speech_finish_kernel (every wave forms the same one-pass statistics, eps
// 1e-5); the normalised row, rounded to the operand dtype TW, is parked in LDS.  Wave w takes candidates w, w + 4, …: lanes split K,
// fp32 products, butterfly add, logit to LDS.  Wave 0 takes the arg-max (ties: the smaller TOKEN ID, what an arg-max over the
// vocabulary row returns, whatever the list's order).  Softmax in fp32: the maximum is subtracted first (every exponent <= 0, an
// offset of the whole row costs nothing) and thread 0 adds the terms in list order, so a row's values do not depend on its batch.
template <typename TW>
__global__ __launch_bounds__(256) void lang_detect_kernel(LangDetectParams p) {
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    __shared__ float s_a[LANG_DETECT_MAX_K];
    __shared__ float s_logit[LANG_DETECT_MAX];
    __shared__ float s_term[LANG_DETECT_MAX];
    __shared__ float s_max, s_sum;
    const float* xr = p.x + (size_t)b * p.ldx;
    float sm = 0.f, sq = 0.f;
    for (int k = lane; k < p.K; k += 64) {
        const float v = xr[k];
        sm += v;
        sq += v * v;
    }
    sm = wave_sum(sm);
    sq = wave_sum(sq);
    const float mean = sm / (float)p.K;
    const float var = (sq / (float)p.K) - (mean * mean);
    const float rstd = 1.0f / sqrtf(fmaxf(var, 0.f) + 1e-5f);
    for (int k = tid; k < p.K; k += 256) s_a[k] = (float)from_f32<TW>((xr[k] - mean) * rstd * p.ln_g[k] + p.ln_b[k]);
    __syncthreads();
    for (int c = w; c < p.n_lang; c += 4) {
        const TW* er = (const TW*)p.emb + (size_t)p.lang_ids[c] * p.K;
        float acc = 0.f;
        for (int k = lane; k < p.K; k += 64) acc += s_a[k] * (float)er[k];
        acc = wave_sum(acc);
        if (lane == 0) s_logit[c] = acc;
    }
    __syncthreads();
    if (w == 0) {
        // (starts at a list member: with NaN logits no comparison holds, and the id written to the prompt table must still be a
        //  vocabulary id)
        float bv = -INFINITY;
        int bi = p.lang_ids[0];
        for (int c = lane; c < p.n_lang; c += 64) {
            const float v = s_logit[c];
            const int id = p.lang_ids[c];
            if (v > bv || (v == bv && id < bi)) {
                bv = v;
                bi = id;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float v2 = __shfl_xor(bv, o, 64);
            const int i2 = __shfl_xor(bi, o, 64);
            if (v2 > bv || (v2 == bv && i2 < bi)) {
                bv = v2;
                bi = i2;
            }
        }
        if (lane == 0) {
            s_max = bv;
            p.lang_out[b] = bi;
            if (p.patch) p.patch[(size_t)b * p.patch_stride + p.patch_col[b]] = bi;
        }
    }
    __syncthreads();
    if (tid < p.n_lang) s_term[tid] = expf(s_logit[tid] - s_max);
    __syncthreads();
    if (tid == 0) {
        float S = 0.f;
        for (int c = 0; c < p.n_lang; ++c) S += s_term[c];  // finite logits: S >= 1, the winner's term is exp(0) (NaN logits give NaN probabilities)
        s_sum = S;
    }
    __syncthreads();
    if (p.probs && tid < p.n_lang) p.probs[(size_t)b * p.n_lang + tid] = s_term[tid] / s_sum;
}
template <typename TW> void launch_lang_detect(const LangDetectParams& p, hipStream_t st) {
    hipLaunchKernelGGL(lang_detect_kernel<TW>, dim3(p.B), dim3(256), 0, st, p);
}
template void launch_lang_detect<float>(const LangDetectParams&, hipStream_t);
template void launch_lang_detect<bf16>(const LangDetectParams&, hipStream_t);
template void launch_lang_detect<f16>(const LangDetectParams&, hipStream_t);

// ------------------------------------------------------------------------------------------------------------
// op-level helpers (known-answer tests of the C-ABI)
__global__ void gelu_kernel(float* t, size_t n, int mode) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) t[i] = gelu_f(t[i], mode);
}
void launch_gelu(float* t, size_t n, int mode, hipStream_t st) {
    // the reference leaves the tail t.size % width untouched (whisper_tensor.mojo:308); width = 8 (x86 AVX2 lanes)
    size_t nb = (n / 8) * 8;
    if (nb) hipLaunchKernelGGL(gelu_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, t, nb, mode);
}
// 3-pass row softmax (whisper_tensor.mojo:311-355), one wave per row
__global__ __launch_bounds__(256) void softmax_rows_kernel(float* t, int rows, int cols) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float* r = t + (size_t)row * cols;
    float mx = -INFINITY;
    for (int j = lane; j < cols; j += 64) mx = fmaxf(mx, r[j]);
    mx = wave_max(mx);
    float s = 0.f;
    for (int j = lane; j < cols; j += 64) {
        float e = expf(r[j] - mx);
        r[j] = e;
        s += e;
    }
    s = wave_sum(s);
    for (int j = lane; j < cols; j += 64) r[j] = r[j] / s;
}
void launch_softmax_rows(float* t, int rows, int cols, hipStream_t st) {
    hipLaunchKernelGGL(softmax_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, t, rows, cols);
}
template <typename T> __global__ void convert_kernel(const float* in, T* out, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = from_f32<T>(in[i]);
}
template <typename T> void launch_convert(const float* in, void* out, size_t n, hipStream_t st) {
    hipLaunchKernelGGL(convert_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, in, (T*)out, n);
}
template void launch_convert<float>(const float*, void*, size_t, hipStream_t);
template void launch_convert<bf16>(const float*, void*, size_t, hipStream_t);
template void launch_convert<f16>(const float*, void*, size_t, hipStream_t);
__global__ void transpose_f32_kernel(const float* in, float* out, int rows, int cols) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (size_t)rows * cols) {
        int r = (int)(i / cols), c = (int)(i % cols);
        out[(size_t)c * rows + r] = in[i];
    }
}
void launch_transpose_f32(const float* in, float* out, int rows, int cols, hipStream_t st) {
    size_t n = (size_t)rows * cols;
    hipLaunchKernelGGL(transpose_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, in, out, rows, cols);
}

}  // namespace wm
