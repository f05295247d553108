// kernels_score.hip — teacher-forced scoring of a given transcript: the vocabulary side of a pass that has
// M = Σ_b (len_b − 1) hidden rows at once and needs two scalars per row, never an M x vocab matrix.
//
//   score_collect   the real rows of a position-major prefill chunk -> the pass's row buffer [M][d]
//   score_ln        the final LayerNorm of the M rows, ONCE, written in the operand form the sweep multiplies: TW rows for 16-bit
//                   decoders and for fp32 at d >= 512, the three bf16 images (x = h + m + l by truncation, dec_logits_split_kernel's
//                   split) for fp32 at d = 128 / 384.  Statistics and rounding are those of the decode step's logits kernels
//                   (8 threads per row, thread q sums the float4 groups q + 8·i in order, three butterfly adds).
//   score_logits    grid (vocabulary parts, row blocks of 128).  Wave w of a workgroup keeps the operand fragments of its 16 rows in
//                   registers for the whole kernel (d = 1024: half a row at a time, re-read per staged unit; ScoreCfg::NP); the workgroup stages the embedding 64 (16-bit) / 32 (fp32) columns at a time
//                   into LDS — fp32 weights on the split path are split once while they are staged — and every wave multiplies the
//                   staged columns with its rows, so each embedding byte that arrives from HBM or the Infinity Cache serves 128 rows.
//                   Per lane a running (max, Σ exp(v − max), arg-max, target logit) over its 4 columns of every tile; the four lanes
//                   of a row meet by two butterfly steps; one (max, sum, arg-max) per (row, part) is stored, and the lane that owns
//                   the row's target column stores that logit.
//   score_merge     per row: the parts in ascending order, logprob = (z_target − max) − log Σ, the arg-max with the lowest id on
//                   ties; score_sums adds each utterance's scored positions in ascending order.
//
// The part boundaries depend on the vocabulary size and the dtype only, never on M, and a row's arithmetic never reads another row:
// a row scored in any batch gives the same bits.
#include "wm_kernels.h"

#include <climits>

namespace wm {

__global__ void score_collect_kernel(const float* __restrict__ rows, float* __restrict__ out, const int* __restrict__ dst, int n_rows, int d4) {
    const int r = blockIdx.x;
    if (r >= n_rows) return;
    const int o = dst[r];
    if (o < 0) return;
    const f32x4* s = reinterpret_cast<const f32x4*>(rows) + (size_t)r * d4;
    f32x4* t = reinterpret_cast<f32x4*>(out) + (size_t)o * d4;
    for (int i = threadIdx.x; i < d4; i += blockDim.x) t[i] = s[i];
}
void launch_score_collect(const float* rows, float* out, const int* dst, int n_rows, int d, hipStream_t st) {
    hipLaunchKernelGGL(score_collect_kernel, dim3(n_rows), dim3(128), 0, st, rows, out, dst, n_rows, d / 4);
}

// ---- final LayerNorm, once per row ----------------------------------------------------------------------------------------
template <typename TW, int KD, bool SPLIT>
__global__ __launch_bounds__(256) void score_ln_kernel(const float* __restrict__ x, const float* __restrict__ ln_g, const float* __restrict__ ln_b,
                                                       void* __restrict__ out, int M) {
    constexpr int K = KD * 128;
    const int row = blockIdx.x * 32 + (threadIdx.x >> 3), q = threadIdx.x & 7;
    const int rr = min(row, M - 1);  // (whole 8-lane groups stay converged for the butterfly; a clamped row stores nothing)
    const float* xr = x + (size_t)rr * K;
    f32x4 v[KD * 4];
#pragma unroll
    for (int i = 0; i < KD * 4; ++i) v[i] = *reinterpret_cast<const f32x4*>(xr + 4 * (q + 8 * i));
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
    if (row >= M) return;
#pragma unroll
    for (int i = 0; i < KD * 4; ++i) {
        const int k = 4 * (q + 8 * i);
        const f32x4 gm = *reinterpret_cast<const f32x4*>(ln_g + k), bt = *reinterpret_cast<const f32x4*>(ln_b + k);
        if constexpr (SPLIT) {
            typedef __attribute__((ext_vector_type(4))) unsigned short u16x4;
            u16x4 oh, om, ol;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float y = (v[i][j] - mean) * rstd * gm[j] + bt[j];
                const unsigned uh = __float_as_uint(y) & 0xffff0000u;
                const float r1 = y - __uint_as_float(uh);
                const unsigned um = __float_as_uint(r1) & 0xffff0000u;
                const float r2 = r1 - __uint_as_float(um);
                oh[j] = (unsigned short)(uh >> 16);
                om[j] = (unsigned short)(um >> 16);
                ol[j] = (unsigned short)(__float_as_uint(r2) >> 16);
            }
            unsigned short* o16 = reinterpret_cast<unsigned short*>(out);
            const size_t img = (size_t)M * K, at = (size_t)row * K + k;
            *reinterpret_cast<u16x4*>(o16 + at) = oh;
            *reinterpret_cast<u16x4*>(o16 + img + at) = om;
            *reinterpret_cast<u16x4*>(o16 + 2 * img + at) = ol;
        } else {
            typedef __attribute__((ext_vector_type(4))) TW t4;
            t4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = from_f32<TW>((v[i][j] - mean) * rstd * gm[j] + bt[j]);
            *reinterpret_cast<t4*>(reinterpret_cast<TW*>(out) + (size_t)row * K + k) = o;
        }
    }
}

// ---- the sweep ------------------------------------------------------------------------------------------------------------
template <typename TW, int KD, bool SPLIT> struct ScoreCfg {
    static constexpr int K = KD * 128;
    static constexpr int KS = KD * 4;                          // k-steps of 32
    static constexpr int CS = sizeof(TW) == 2 ? 4 : 2;         // column tiles (of 16) per stage
    // column tiles staged (and held in flight as `pre`) together.  fp32 rows of d_model 768 keep 24 fragments = 192 VGPRs per lane for
    // the whole kernel: a stage goes through LDS one tile at a time there, in the same tile order — stages, parts and every row's
    // arithmetic are what two tiles at once would give — and a tile is fetched when it is parked, not a tile ahead: 24 VGPRs of
    // prefetch held across the MFMAs were 15 more than the 256 a 512-thread workgroup leaves a wave (60 bytes of scratch).  The
    // sweep issues 192 MFMAs of 32 cycles per tile and wave with fp32 operands, so the exposed round trip is expected to be the smaller
    // part; that has not been measured
    static constexpr int CSU = (sizeof(TW) == 4 && !SPLIT && KD > 4) ? 1 : CS;
    // d_model 1024 (32 k-steps): a row is 32 fragments — 256 VGPRs in fp32, 128 in 16-bit next to 64 of prefetch and the ~100 the rest
    // of the sweep takes — so it is NOT held.  K is walked in NP = 2 halves: for each staged unit a wave fetches the first half of its
    // 16 rows (16 fragments, from L2: score_ln wrote them just before), multiplies every tile of the unit by it, fetches the second half
    // into the same registers and carries each tile's accumulator on.  A tile's k-steps still enter its accumulator in the order
    // 0, 1, ..., 31, so the bits are those of a held row.  (Rows in LDS instead: 128 x 1024 is 256 KB in 16-bit — no room.)
    static constexpr int NP = KD > 6 ? 2 : 1;
    static constexpr int KSP = KS / NP;                        // k-steps of a wave's rows in registers together
    static_assert(!(SPLIT && NP > 1), "the split images are held whole");
    static constexpr int SUB = CS / CSU;                       // staged units per stage
    static constexpr int COLS = CSU * 16;
    static constexpr int ESZ = SPLIT ? 2 : (int)sizeof(TW);    // bytes per LDS element
    // LDS row pitch in elements: 16-bit images ≡ 8 dwords (mod 64), as dec_logits_split_kernel's; fp32 rows + 16 bytes
    static constexpr int PITCH = ESZ == 2 ? K + 16 : K + 4;
    static constexpr int CPR = K * (int)sizeof(TW) / 16;       // 16-byte chunks per embedding row
    static constexpr int NCH = COLS * CPR / 512;               // chunks of a stage per thread
    static constexpr size_t LDS = (size_t)(SPLIT ? 3 : 1) * COLS * PITCH * ESZ;
    static_assert(COLS * CPR % 512 == 0, "a stage must divide over the workgroup");
};
static const int SCORE_ROWS = 128;       // rows per workgroup
static const int SCORE_MAX_PARTS = 32;   // vocabulary parts: a function of N and the dtype alone

struct ScoreSweepParams {
    const void* a;      // score_ln's output
    const void* W;      // [N][K] operand dtype
    const int* target;  // [M]; < 0: no target logit
    int M, N;
    int parts, spp;     // parts, stages per part
    float* pmax;        // [M][parts]
    float* psum;
    int* pidx;
    float* ztgt;        // [M]
};

// one tile into a lane's running (max, Σ exp, arg-max, target logit): acc[r] = logit[row][n0 + 4 g + r].  Text, not a function: both forms
// of the sweep below expand it, and the held-row form compiles to what it was before the second form existed.
#define WM_SCORE_FOLD(n0, acc)                                                                                                   \
    do {                                                                                                                         \
        float v[4];                                                                                                              \
        float mt = m; /* the maximum after this tile */                                                                          \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                                          \
            const int n = (n0) + 4 * g + r;                                                                                      \
            v[r] = n < p.N ? (acc)[r] : -INFINITY;                                                                               \
            if (n == tgt) {                                                                                                      \
                zt = (acc)[r];                                                                                                   \
                got = true;                                                                                                      \
            }                                                                                                                    \
            if (v[r] > mt) { /* n grows along the loop: strict '>' keeps the lowest id */                                        \
                mt = v[r];                                                                                                       \
                bi = n;                                                                                                          \
            }                                                                                                                    \
        }                                                                                                                        \
        if (mt > m) { /* the sum follows the maximum once per tile.  (the s > 0 guards here and in the merges keep */            \
            s = s > 0.f ? s * expf(m - mt) : 0.f; /* expf(-inf - -inf) = NaN out while nothing has been summed yet) */           \
            m = mt;                                                                                                              \
        }                                                                                                                        \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) if (v[r] > -INFINITY) s += expf(v[r] - m);                                 \
    } while (0)

template <typename TW, int KD, bool SPLIT>
__global__ __launch_bounds__(512) void score_logits_kernel(ScoreSweepParams p) {
    using C = ScoreCfg<TW, KD, SPLIT>;
    constexpr int K = C::K, KS = C::KS, PITCH = C::PITCH;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int row = blockIdx.y * SCORE_ROWS + w * 16 + r16;
    const int rr = min(row, p.M - 1);  // a ragged block's spare lanes multiply the last row again and store nothing
    const int tiles = (p.N + 15) / 16;
    const int stages = (tiles + C::CS - 1) / C::CS;
    // (score_parts never yields an empty part — (parts - 1)·spp < stages — so st_lo < st_hi for every launch of launch_score; the
    //  guards below only keep a launcher with another partition from storing uninitialised partials)
    const int st_lo = blockIdx.x * p.spp, st_hi = min(stages, st_lo + p.spp);

    // this wave's rows as MFMA operand fragments, for the whole kernel
    Frag<TW> af[SPLIT ? 1 : C::KSP];
    bf16x8 ah[SPLIT ? KS : 1], am[SPLIT ? KS : 1], al[SPLIT ? KS : 1];
    if constexpr (SPLIT) {
        const bf16* a = reinterpret_cast<const bf16*>(p.a) + (size_t)rr * K + g * 8;
        const size_t img = (size_t)p.M * K;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            ah[ks] = *reinterpret_cast<const bf16x8*>(a + ks * 32);
            am[ks] = *reinterpret_cast<const bf16x8*>(a + img + ks * 32);
            al[ks] = *reinterpret_cast<const bf16x8*>(a + 2 * img + ks * 32);
        }
    } else if constexpr (C::NP == 1) {
        const TW* a = reinterpret_cast<const TW*>(p.a) + (size_t)rr * K + g * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) af[ks] = load_frag<TW>(a + ks * 32);
    }
    const int tgt = p.target[rr];

    // one stage of embedding rows: global -> registers (in flight during the previous stage's MFMAs) -> LDS
    f32x4 pre[C::NCH];
    auto fetch = [&](int unit) {
#pragma unroll
        for (int i = 0; i < C::NCH; ++i) {
            const int c = threadIdx.x + i * 512;
            const int col = c / C::CPR, off = c % C::CPR;
            const int n = min(unit * C::COLS + col, p.N - 1);  // columns past N re-read the last row; the epilogue drops them
            pre[i] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const unsigned char*>(p.W) + ((size_t)n * C::CPR + off) * 16);
        }
    };
    auto park = [&]() {
#pragma unroll
        for (int i = 0; i < C::NCH; ++i) {
            const int c = threadIdx.x + i * 512;
            const int col = c / C::CPR, off = c % C::CPR;
            if constexpr (SPLIT) {
                typedef __attribute__((ext_vector_type(4))) unsigned short u16x4;
                u16x4 oh, om, ol;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float y = pre[i][j];
                    const unsigned uh = __float_as_uint(y) & 0xffff0000u;
                    const float r1 = y - __uint_as_float(uh);
                    const unsigned um = __float_as_uint(r1) & 0xffff0000u;
                    const float r2 = r1 - __uint_as_float(um);
                    oh[j] = (unsigned short)(uh >> 16);
                    om[j] = (unsigned short)(um >> 16);
                    ol[j] = (unsigned short)(__float_as_uint(r2) >> 16);
                }
                unsigned short* xs = reinterpret_cast<unsigned short*>(smem_raw);
                const int at = col * PITCH + off * 4;
                *reinterpret_cast<u16x4*>(xs + at) = oh;
                *reinterpret_cast<u16x4*>(xs + C::COLS * PITCH + at) = om;
                *reinterpret_cast<u16x4*>(xs + 2 * C::COLS * PITCH + at) = ol;
            } else {
                *reinterpret_cast<f32x4*>(smem_raw + (size_t)col * PITCH * C::ESZ + (size_t)off * 16) = pre[i];
            }
        }
    };

    float m = -INFINITY, s = 0.f, zt = 0.f;  // running max = the best value so far, Σ exp(v − m), target logit
    int bi = INT_MAX;
    bool got = false;
    // staged units of CSU tiles: SUB per stage (1 everywhere but fp32 at d_model 768), none past the vocabulary's last tile
    const int u_lo = st_lo * C::SUB, u_hi = min(st_hi * C::SUB, (tiles + C::CSU - 1) / C::CSU);
    constexpr bool AHEAD = C::SUB == 1;  // the next unit's rows in flight during this unit's MFMAs
    if (AHEAD && u_lo < u_hi) fetch(u_lo);
    for (int stg = u_lo; stg < u_hi; ++stg) {
        if (!AHEAD) fetch(stg);
        __syncthreads();  // every wave is past the previous unit's fragment reads
        park();
        __syncthreads();
        if (AHEAD && stg + 1 < u_hi) fetch(stg + 1);
        if constexpr (C::NP > 1) {  // K in halves: this wave's rows, half by half, through every tile of the unit
            const TW* a = reinterpret_cast<const TW*>(p.a) + (size_t)rr * K + g * 8;
            f32x4 accs[C::CSU];
#pragma unroll
            for (int t = 0; t < C::CSU; ++t) accs[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int h = 0; h < C::NP; ++h) {
#pragma unroll
                for (int ks = 0; ks < C::KSP; ++ks) af[ks] = load_frag<TW>(a + (h * C::KSP + ks) * 32);
#pragma unroll
                for (int t = 0; t < C::CSU; ++t) {
                    if ((stg * C::CSU + t) * 16 >= p.N) break;  // workgroup-uniform: no MFMAs for a tile past the vocabulary
                    const TW* xs = reinterpret_cast<const TW*>(smem_raw) + (t * 16 + r16) * PITCH + g * 8 + h * C::KSP * 32;
#pragma unroll
                    for (int ks = 0; ks < C::KSP; ++ks) accs[t] = mma32(load_frag<TW>(xs + ks * 32), af[ks], accs[t]);
                }
            }
#pragma unroll
            for (int t = 0; t < C::CSU; ++t) {
                const int n0 = (stg * C::CSU + t) * 16;
                if (n0 >= p.N) break;  // workgroup-uniform
                WM_SCORE_FOLD(n0, accs[t]);
            }
        } else {
#pragma unroll
        for (int t = 0; t < C::CSU; ++t) {
            const int n0 = (stg * C::CSU + t) * 16;
            if (n0 >= p.N) break;  // workgroup-uniform
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (SPLIT) {
                const bf16* xs = reinterpret_cast<const bf16*>(smem_raw) + (t * 16 + r16) * PITCH + g * 8;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {  // the six products of dec_logits_split_kernel, smallest terms first
                    const bf16x8 wh = *reinterpret_cast<const bf16x8*>(xs + ks * 32);
                    const bf16x8 wm_ = *reinterpret_cast<const bf16x8*>(xs + C::COLS * PITCH + ks * 32);
                    const bf16x8 wl = *reinterpret_cast<const bf16x8*>(xs + 2 * C::COLS * PITCH + ks * 32);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl, ah[ks], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, al[ks], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wm_, am[ks], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wm_, ah[ks], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, am[ks], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, ah[ks], acc, 0, 0, 0);
                }
            } else {
                const TW* xs = reinterpret_cast<const TW*>(smem_raw) + (t * 16 + r16) * PITCH + g * 8;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) acc = mma32(load_frag<TW>(xs + ks * 32), af[ks], acc);
            }
            WM_SCORE_FOLD(n0, acc);
        }
        }
    }
    // the four lanes of a row (symmetric, so all four end with the same values)
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
        const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
        const int i2 = __shfl_xor(bi, o, 64);
        const float mn = fmaxf(m, m2);
        const float sa = s > 0.f ? s * expf(m - mn) : 0.f, sb = s2 > 0.f ? s2 * expf(m2 - mn) : 0.f;
        s = sa + sb;
        if (m2 > m || (m2 == m && i2 < bi)) bi = i2;
        m = mn;
    }
    if (row < p.M) {
        if (g == 0) {
            const size_t o = (size_t)row * p.parts + blockIdx.x;
            p.pmax[o] = m;
            p.psum[o] = s;
            p.pidx[o] = bi;
        }
        if (got) p.ztgt[row] = zt;
    }
}

#undef WM_SCORE_FOLD
int score_parts(int N, int dtype, int* spp_out) {
    const int cs = dtype == 0 ? 2 : 4;
    const int tiles = (N + 15) / 16, stages = (tiles + cs - 1) / cs;
    const int spp = (stages + SCORE_MAX_PARTS - 1) / SCORE_MAX_PARTS;
    if (spp_out) *spp_out = spp;
    return (stages + spp - 1) / spp;
}

struct ScoreMergeParams {
    const float* pmax;
    const float* psum;
    const int* pidx;
    const float* ztgt;
    const int* target;
    const int* slot;  // [M] where row r's results go in the tables, or null: r
    int M, parts;
    float* logprob;
    int* top_id;  // or null
};
__global__ void score_merge_kernel(ScoreMergeParams p) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= p.M) return;
    const float* pm = p.pmax + (size_t)r * p.parts;
    const float* ps = p.psum + (size_t)r * p.parts;
    const int* pi = p.pidx + (size_t)r * p.parts;
    float mx = -INFINITY;
    int bi = INT_MAX;
    for (int k = 0; k < p.parts; ++k) {
        const float v = pm[k];
        const int i = pi[k];
        if (v > mx || (v == mx && i < bi)) {
            mx = v;
            bi = i;
        }
    }
    float S = 0.f;
    for (int k = 0; k < p.parts; ++k)
        if (ps[k] > 0.f) S += ps[k] * expf(pm[k] - mx);
    const int o = p.slot ? p.slot[r] : r;
    p.logprob[o] = p.target[r] >= 0 ? (p.ztgt[r] - mx) - logf(S) : 0.f;  // the maxima leave first, as in argmax_step
    if (p.top_id) p.top_id[o] = bi == INT_MAX ? 0 : bi;
}
// per utterance: Σ logprob[b][t] over ctx[b] <= t < len[b], ascending, and its mean
__global__ void score_sums_kernel(const float* __restrict__ logprob, int stride, const int* __restrict__ len, const int* __restrict__ ctx,
                                  float* __restrict__ sum, float* __restrict__ avg, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float s = 0.f;
    for (int t = ctx[b]; t < len[b]; ++t) s += logprob[(size_t)b * stride + t];
    sum[b] = s;
    avg[b] = s / (float)(len[b] - ctx[b]);
}
void launch_score_sums(const float* logprob, int stride, const int* len, const int* ctx, float* sum, float* avg, int B, hipStream_t st) {
    hipLaunchKernelGGL(score_sums_kernel, dim3((B + 127) / 128), dim3(128), 0, st, logprob, stride, len, ctx, sum, avg, B);
}

// n-best scoring: one workgroup per clip.  Candidate c of the clip (key[row0 + c]) gets
//   rank_c = #{j : key_j > key_c or (key_j == key_c and j < c)}   — a permutation of 0 .. n - 1, so order[row0 + rank_c] = c has no
//   write conflict: no sort network, no atomics —
//   posterior_c = expf(key_c - M) / Σ_j expf(key_j - M),  M = the clip's largest key, the sum in ascending j.
// Every thread walks the clip's keys itself (n <= max_batch values, wave-uniform loads): no LDS, no barrier, and the same sum in
// every thread, whatever the other clips of the launch hold.  Keys are finite or -inf below a finite maximum (log-prob sums); a NaN
// key compares false everywhere, so NaN candidates would all take rank 0 and leave other order entries unwritten — every store
// still lands inside the clip's rows, and wm_op_score_rank refuses such keys.
__global__ __launch_bounds__(64) void score_rank_kernel(ScoreRankParams p) {
    const int u = blockIdx.x, r0 = p.row0[u], n = p.n_cand[u];
    const float* key = p.key + r0;
    float M = key[0];
    for (int j = 1; j < n; ++j) M = fmaxf(M, key[j]);
    float S = 0.f;
    for (int j = 0; j < n; ++j) S += expf(key[j] - M);
    for (int c = threadIdx.x; c < n; c += blockDim.x) {
        const float kc = key[c];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const float kj = key[j];
            rank += (kj > kc || (kj == kc && j < c)) ? 1 : 0;
        }
        p.order[r0 + rank] = c;
        if (rank == 0) p.best[u] = c;
        p.posterior[r0 + c] = expf(kc - M) / S;
    }
}
void launch_score_rank(const ScoreRankParams& p, int U, hipStream_t st) { hipLaunchKernelGGL(score_rank_kernel, dim3(U), dim3(64), 0, st, p); }

template <typename TW, int KD, bool SPLIT> static int score_run(const ScoreParams& q, hipStream_t st, hipEvent_t* ev) {
    using C = ScoreCfg<TW, KD, SPLIT>;
    hipLaunchKernelGGL((score_ln_kernel<TW, KD, SPLIT>), dim3((q.M + 31) / 32), dim3(256), 0, st, q.x, q.ln_g, q.ln_b, q.a, q.M);
    if (ev) (void)hipEventRecord(ev[0], st);
    if (C::LDS > 48 * 1024)
        if (const hipError_t e = ensure_dyn_lds<&score_logits_kernel<TW, KD, SPLIT>>((int)C::LDS); e != hipSuccess)
            return launch_hip_failed("score_logits kernel: dynamic LDS attribute", e);
    ScoreSweepParams p{};
    p.a = q.a;
    p.W = q.emb;
    p.target = q.target;
    p.M = q.M;
    p.N = q.N;
    p.parts = score_parts(q.N, sizeof(TW) == 4 ? 0 : 1, &p.spp);
    p.pmax = q.pmax;
    p.psum = q.psum;
    p.pidx = q.pidx;
    p.ztgt = q.ztgt;
    hipLaunchKernelGGL((score_logits_kernel<TW, KD, SPLIT>), dim3(p.parts, (q.M + SCORE_ROWS - 1) / SCORE_ROWS), dim3(512), C::LDS, st, p);
    if (ev) (void)hipEventRecord(ev[1], st);
    ScoreMergeParams mp{};
    mp.pmax = q.pmax;
    mp.psum = q.psum;
    mp.pidx = q.pidx;
    mp.ztgt = q.ztgt;
    mp.target = q.target;
    mp.slot = q.slot;
    mp.M = q.M;
    mp.parts = p.parts;
    mp.logprob = q.logprob;
    mp.top_id = q.top_id;
    hipLaunchKernelGGL(score_merge_kernel, dim3((q.M + 127) / 128), dim3(128), 0, st, mp);
    return WM_LAUNCH_OK;
}
size_t score_operand_bytes(int M, int K, int dtype) { return (size_t)M * K * (dtype == 0 ? (K >= 512 ? 4 : 6) : 2); }
template <typename TW> int launch_score(const ScoreParams& q, hipStream_t st, hipEvent_t* ev) {
    const int kd = q.K >> 7;
    if (q.M <= 0 || q.N <= 0) return launch_refuse("score: empty problem");
    if ((q.K & 127) != 0 || (kd != 1 && kd != 3 && kd != 4 && kd != 6 && kd != 8)) return launch_refuse("score: d_model must be 128, 384, 512, 768 or 1024");
    if constexpr (sizeof(TW) == 4) {
        if (kd == 1) return score_run<float, 1, true>(q, st, ev);
        if (kd == 3) return score_run<float, 3, true>(q, st, ev);
        if (kd == 6) return score_run<float, 6, false>(q, st, ev);  // exact fp32, as d_model 512 and as the decode step's logits at 768
        if (kd == 8) return score_run<float, 8, false>(q, st, ev);  // exact fp32 too, K in two halves
        return score_run<float, 4, false>(q, st, ev);
    } else {
        if (kd == 1) return score_run<TW, 1, false>(q, st, ev);
        if (kd == 3) return score_run<TW, 3, false>(q, st, ev);
        if (kd == 6) return score_run<TW, 6, false>(q, st, ev);
        if (kd == 8) return score_run<TW, 8, false>(q, st, ev);
        return score_run<TW, 4, false>(q, st, ev);
    }
}
template int launch_score<float>(const ScoreParams&, hipStream_t, hipEvent_t*);
template int launch_score<bf16>(const ScoreParams&, hipStream_t, hipEvent_t*);
template int launch_score<f16>(const ScoreParams&, hipStream_t, hipEvent_t*);

}  // namespace wm
