// xattn_sweep.inc — the body of the X sweep (see kernels_decoder.hip, "The X sweep"), included once per kernel form so that every form is
// the same statements: XATTN_UTT(slot) names the clip whose X the row in batch slot `slot` sweeps.  Expects H, NT and p in scope.
    constexpr int D = 64 * H, NKS = D / 32, NDB = D / 16;
    constexpr int XP = D + 16;  // row pitch (elements): 32·H + 8 dwords, so the 8 rows of one transposed read hit disjoint banks
    __shared__ __attribute__((aligned(16))) bf16 sQ[3 * (H + 1) * XP];  // q' images; row H of each image is zero
    __shared__ __attribute__((aligned(16))) bf16 sX[4 * 16 * XP];        // per wave: the parked 16-key tile; at the end: Y of 4 waves
    __shared__ float sML[4][H][2];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r16 = lane & 15, g = lane >> 4;
    const int split = blockIdx.x, row = blockIdx.y;
    const int utt = XATTN_UTT(p.q_B > 0 ? row % p.q_B : row);
    const int len = p.n_keys, chunk = (len + p.nsplit - 1) / p.nsplit;
    const int j0 = split * chunk, j1 = min(len, j0 + chunk);
    const int hq = r16 < H ? r16 : H;
    const bf16* X = (const bf16*)p.X + (size_t)utt * p.x_stride;
    bf16* park = sX + w * 16 * XP;
    const int ntile = j1 > j0 ? (j1 - j0 + 15) / 16 : 0;

    auto load = [&](bf16x8 (&xr)[NKS], int t) {
        const int key = max(min(j0 + 16 * t + r16, j1 - 1), 0);
        const bf16* src = X + (size_t)key * D + g * 8;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            if (NT)
                xr[ks] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(src + ks * 32));
            else
                xr[ks] = *reinterpret_cast<const bf16x8*>(src + ks * 32);
        }
    };
    // the wave's first X tile is requested before anything else: the q' staging and its barrier run under that round trip
    bf16x8 xa[NKS], xb[NKS];
    if (w < ntile) load(xa, w);
    {  // q' images -> sQ: a thread owns one 16-byte column of every RPP-th (image, head) row, so its index split is done once
        constexpr int C8 = D / 8, RPP = 256 / C8;
        static_assert(RPP >= 3, "the three zero rows are filled by the first three row slots");
        const bf16x8* src = (const bf16x8*)((const bf16*)p.qs + (size_t)row * 3 * H * D);
        const int sr = threadIdx.x / C8, sc = threadIdx.x % C8;
        if (sr < RPP) {
#pragma unroll
            for (int rr = sr; rr < 3 * H; rr += RPP) {
                const int img = rr / H, hh = rr - img * H;
                *reinterpret_cast<bf16x8*>(&sQ[(img * (H + 1) + hh) * XP + sc * 8]) = src[rr * C8 + sc];
            }
            if (sr < 3) *reinterpret_cast<bf16x8*>(&sQ[(sr * (H + 1) + H) * XP + sc * 8]) = bf16x8{};
        }
    }
    __syncthreads();
    f32x4 y[NDB];
#pragma unroll
    for (int db = 0; db < NDB; ++db) y[db] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -1e10f, l_run = 0.f;
    auto consume = [&](const bf16x8 (&xr)[NKS], int t) {
        // one accumulator per q' term: three independent MFMA chains of NKS instead of one dependent chain of 3·NKS
        f32x4 sk[3] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const bf16x8 qf = *reinterpret_cast<const bf16x8*>(&sQ[(k * (H + 1) + hq) * XP + ks * 32 + g * 8]);
                sk[k] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xr[ks], qf, sk[k], 0, 0, 0);
            }
        const f32x4 s = (sk[0] + sk[1]) + sk[2];
        // lane (head r16, group g) holds the scores of keys 4g..4g+3 of the tile
        const int kb = j0 + 16 * t + 4 * g;
        float sc[4], bm = -1e30f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            sc[r] = kb + r < j1 ? s[r] : -1e30f;
            bm = fmaxf(bm, sc[r]);
        }
        bm = fmaxf(bm, __shfl_xor(bm, 16, 64));
        bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
        const float m_new = fmaxf(m_run, bm);
        const float alpha = expf(m_run - m_new);
        float pe[4], ps = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            pe[r] = expf(sc[r] - m_new);
            ps += pe[r];
        }
        ps += __shfl_xor(ps, 16, 64);
        ps += __shfl_xor(ps, 32, 64);
        l_run = l_run * alpha + ps;
        m_run = m_new;
        typedef __attribute__((ext_vector_type(4))) unsigned short u16x4;
        u16x4 ph, pm, pl;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            unsigned short a, b, c;
            split3_1(pe[r], a, b, c);
            ph[r] = a;
            pm[r] = b;
            pl[r] = c;
        }
        const bf16x4 fh = __builtin_bit_cast(bf16x4, ph), fm = __builtin_bit_cast(bf16x4, pm), fl = __builtin_bit_cast(bf16x4, pl);
        wave_lds_fence();  // the previous tile's transposed reads are done
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) *reinterpret_cast<bf16x8*>(&park[r16 * XP + ks * 32 + g * 8]) = xr[ks];
        wave_lds_fence();
#pragma unroll
        for (int db = 0; db < NDB; ++db) {
            const bf16x4 xt = lds_tr16_bf16(&park[(4 * g + (r16 >> 2)) * XP + db * 16 + (r16 & 3) * 4]);
            f32x4 a = y[db] * alpha;
            a = mma16_bf16(xt, fh, a);
            a = mma16_bf16(xt, fm, a);
            y[db] = mma16_bf16(xt, fl, a);
        }
    };

    if (w < ntile) {
        int t = w;
        while (true) {
            const bool more1 = t + 4 < ntile;
            if (more1) load(xb, t + 4);
            consume(xa, t);
            t += 4;
            if (!more1) break;
            const bool more2 = t + 4 < ntile;
            if (more2) load(xa, t + 4);
            consume(xb, t);
            t += 4;
            if (!more2) break;
        }
    }
    // merge the four waves (as attn_decode_kernel merges its row slots), write the chunk's partial
    __syncthreads();
    float* sY = reinterpret_cast<float*>(sX);  // [4][H][D]
    if (r16 < H) {
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int r = 0; r < 4; ++r) sY[(w * H + r16) * D + db * 16 + 4 * g + r] = y[db][r];
        if (g == 0) {
            sML[w][r16][0] = m_run;
            sML[w][r16][1] = l_run;
        }
    }
    __syncthreads();
    const size_t prow = (size_t)row * p.nsplit + split;
    // the four waves' weights of a head: once per head (they were one expf per wave and output element), then 16-byte combines
    __shared__ float sWg[4][H];
    if (threadIdx.x < H) {
        const int h = threadIdx.x;
        float M = -1e10f;
#pragma unroll
        for (int v = 0; v < 4; ++v) M = fmaxf(M, sML[v][h][0]);
        float L = 0.f;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const float wgt = sML[v][h][1] > 0.f ? expf(sML[v][h][0] - M) : 0.f;
            L += wgt * sML[v][h][1];
            sWg[v][h] = wgt;
        }
        p.part_ml[(prow * H + h) * 2] = M;
        p.part_ml[(prow * H + h) * 2 + 1] = L;
    }
    __syncthreads();
    for (int i = threadIdx.x * 4; i < H * D; i += 256 * 4) {
        const int h = i / D;
        f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const float wgt = sWg[v][h];
            const f32x4 yv = *reinterpret_cast<const f32x4*>(&sY[v * H * D + i]);
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] += wgt * yv[k];
        }
        *reinterpret_cast<f32x4*>(p.part_y + prow * H * D + i) = o;
    }
