// vq_stream.inc -- exact nearest-codeword search for codebooks that do not fit LDS (included from vq.hip).
//
// Same contract and the same bits as the resident kernels of vq.hip (msmc_vq_search), but one head's codebook is never
// resident: it passes through LDS in chunks of Kc codewords -- rows [Kc][d] at the resident kernels' pitch d + 4, plus the
// Kc norms -- in two buffers.  While the workgroup searches chunk q in one buffer, the rows of chunk q + 1 travel
// HBM / L2 -> registers (loads issued ahead of each 32-codeword MFMA step) -> the other buffer (stores behind that step);
// one workgroup barrier per chunk closes the hand-over.  The chunk sequence is (head 0: chunks 0 .. nch-1), (head 1: ...),
// ... and wraps to head 0 for the workgroup's next 64-frame iteration, so the stream never drains inside a launch.
//
// A wave keeps its 16-frame tile for the whole pass over K and carries a running (best distance, best index) per lane
// across the chunks of a head (vq_take_min); the four lane groups that share a frame are merged after the head's last chunk
// (vq_merge_groups).  The winner rows then come from global memory (embed_t, in L2) and quant / diff are formed by
// vq_st_piece.  All of it is vq_common.inc, shared with the resident kernels.
//
// Two instantiation families mirror the two resident kernels, so that the fp32 summation order over the d channels -- and with
// it every bit of the result -- is the one msmc_vq_search uses for the same shape:
//   D4H > 0 : d = 16 * D4H, frame values in registers: the register form of vq_common.inc          (vq_search_reg_kernel)
//   D4H = 0 : any d % 4 == 0, the current head's slice of the tile in LDS: the LDS form            (vq_search_kernel)
// No atomics; every global store is a vector-memory store.

#define VQS_MAX_CHUNK 256            // the next chunk's norms ride in at most 4 registers of a 64-wide workgroup

template <int D4H>
__global__ __launch_bounds__(256, D4H > 0 ? 2 : 1) void vq_search_stream_kernel(
    const float* x, const float* __restrict__ embed_t, const float* __restrict__ enorm, float* quant,
    float* __restrict__ diff, int64_t* __restrict__ ind, int N, int D, int H, int K, int Kc, int xt_off) {
    MSMC_DYN_LDS(smem);
    constexpr bool REG = D4H > 0;
    constexpr bool PREF = REG && D4H <= 8;              // next head's / tile's frame values in flight (register budget)
    constexpr bool DREG = REG && D4H <= 8;              // sum of squares over the heads in registers; else it lives in diff
    constexpr int NX = REG ? D4H : 1;
    constexpr int STG = REG ? (D4H >= 2 ? D4H / 2 : 1) : 8;   // 16-byte pieces per work-item staged per 32-codeword step
    constexpr int NEN = REG ? 1 : 4;
    const int d = REG ? 16 * D4H : D / H;
    const int ES = d + 4, dv = d >> 2;
    float* cb = (float*)smem;                           // [2][Kc][ES]
    float* en = cb + (size_t)2 * Kc * ES;               // [2][Kc]
    const int nthr = blockDim.x, tid = threadIdx.x;
    const int nw = nthr >> 6, w = tid >> 6, lane = tid & 63;
    const int f = lane & 15, g = lane >> 4;
    float* xr = REG ? nullptr : (float*)(smem + xt_off) + ((size_t)w * VQ_TILE + f) * ES;   // this lane's frame, current head
    const int nch = (K + Kc - 1) / Kc;
    const int total = H * nch;
    const int numTiles = (N + VQ_TILE - 1) / VQ_TILE;
    const int numIters = (numTiles + nw - 1) / nw;

    f32x4 st[STG];
    auto stage_load = [&](const float* src, int rows, int pos) {
#pragma unroll
        for (int i = 0; i < STG; ++i) {
            const int e = (pos + i) * nthr + tid;
            if (e < rows * dv) st[i] = ((const f32x4*)src)[e];
        }
    };
    auto stage_store = [&](float* dst, int rows, int pos) {
#pragma unroll
        for (int i = 0; i < STG; ++i) {
            const int e = (pos + i) * nthr + tid;
            if (e < rows * dv) {
                const int r = e / dv, c4 = e - r * dv;
                *(f32x4*)(dst + (size_t)r * ES + c4 * 4) = st[i];
            }
        }
    };

    f32x4 xb[NX], xn[PREF ? NX : 1], dacc[DREG ? NX : 1];
    // (the same lambda as in vq_search_reg_kernel, on purpose: profiles/vq_search_refactor.md "The fragment load stays a lambda")
    auto load_frag = [&](f32x4* dst, int tile, int h) {
        const int n = tile * VQ_TILE + f;
#pragma unroll
        for (int t = 0; t < NX; ++t) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (tile < numTiles && n < N) v = *(const f32x4*)(x + (size_t)n * D + h * d + 16 * t + 4 * g);
            dst[t] = v;
        }
    };

    int it = blockIdx.x;
    if (it >= numIters) return;
    {   // chunk 0 of head 0 -> buffer 0
        const int rows = Kc < K ? Kc : K;
        const int cnt = (rows * dv + nthr - 1) / nthr;
        for (int pos = 0; pos < cnt; pos += STG) {
            stage_load(embed_t, rows, pos);
            stage_store(cb, rows, pos);
        }
        for (int e = tid; e < rows; e += nthr) en[e] = enorm[e];
    }
    if constexpr (PREF) load_frag(xn, it * nw + w, 0);
    __syncthreads();

    int buf = 0;
    float xx = 0.f, best = __builtin_inff();
    int bi = 0;
    for (; it < numIters; it += gridDim.x) {
        const int tile = it * nw + w;
        const bool active = tile < numTiles;
        const int n = tile * VQ_TILE + f;
        const bool row_ok = active && n < N;
        for (int q = 0; q < total; ++q) {
            const int h = q / nch, c = q - h * nch, k0 = c * Kc;
            const int rows = K - k0 < Kc ? K - k0 : Kc;
            // the chunk after this one: next chunk of the head, first chunk of the next head, or head 0 for the next iteration
            const bool wrap = q + 1 == total;
            const bool restage = total > 1 && (!wrap || it + (int)gridDim.x < numIters);
            const int qn = wrap ? 0 : q + 1;
            const int hn = qn / nch, k0n = (qn - hn * nch) * Kc;
            const int rowsn = K - k0n < Kc ? K - k0n : Kc;
            const float* srcn = embed_t + ((size_t)hn * K + k0n) * d;
            const float* cbc = cb + (size_t)buf * Kc * ES;
            const float* enc = en + buf * Kc;
            float* cbn = cb + (size_t)(buf ^ 1) * Kc * ES;
            float* enn = en + (buf ^ 1) * Kc;
            const int cnt = restage ? (rowsn * dv + nthr - 1) / nthr : 0;
            int pos = 0;
            float sn[NEN];
#pragma unroll
            for (int i = 0; i < NEN; ++i) {
                const int e = i * nthr + tid;
                sn[i] = (restage && e < rowsn) ? enorm[(size_t)hn * K + k0n + e] : 0.f;
            }

            if (c == 0) {   // a new head: its slice of the tile, |x|^2, a fresh running minimum
                if constexpr (REG) {
                    if constexpr (PREF) {
#pragma unroll
                        for (int t = 0; t < NX; ++t) xb[t] = xn[t];
                        if (h + 1 < H) load_frag(xn, tile, h + 1);
                        else if (it + (int)gridDim.x < numIters) load_frag(xn, (it + gridDim.x) * nw + w, 0);
                    } else {
                        load_frag(xb, tile, h);
                    }
                    xx = vq_sumsq_reg(xb);
                } else {
                    float* xw = (float*)(smem + xt_off) + (size_t)w * VQ_TILE * ES;
                    for (int e = lane; e < VQ_TILE * dv; e += 64) {
                        const int row = e / dv, c4 = e - row * dv;
                        const int nn = tile * VQ_TILE + row;
                        f32x4 v = {0.f, 0.f, 0.f, 0.f};
                        if (active && nn < N) v = *(const f32x4*)(x + (size_t)nn * D + h * d + c4 * 4);
                        *(f32x4*)(xw + (size_t)row * ES + c4 * 4) = v;
                    }
                    wave_sync();             // tile rows were written by other lanes of this wave
                    xx = vq_sumsq_lds(xr, d, g);
                }
                best = __builtin_inff();
                bi = 0;
            }

            if (active) {
                const int ntile = rows >> 4;
                int ct = 0;
                for (; ct + 2 <= ntile; ct += 2) {
                    const bool sg = pos < cnt;
                    if (sg) stage_load(srcn, rowsn, pos);
                    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
                    const float* a0 = cbc + (size_t)(ct * 16 + f) * ES + (REG ? 4 * g : g);
                    if constexpr (REG) vq_dot_reg2(a0, a0 + 16 * ES, xb, acc0, acc1);
                    else vq_dot_lds2(a0, a0 + 16 * ES, xr + g, d, acc0, acc1);
                    const int code0 = ct * 16 + 4 * g;       // position in the chunk: norms by position, indices from k0
                    vq_take_min(acc0, xx, enc + code0, k0 + code0, best, bi);
                    vq_take_min(acc1, xx, enc + code0 + 16, k0 + code0 + 16, best, bi);
                    if (sg) {
                        stage_store(cbn, rowsn, pos);
                        pos += STG;
                    }
                }
                if (ct < ntile) {
                    const bool sg = pos < cnt;
                    if (sg) stage_load(srcn, rowsn, pos);
                    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f};
                    const float* a0 = cbc + (size_t)(ct * 16 + f) * ES + (REG ? 4 * g : g);
                    if constexpr (REG) vq_dot_reg(a0, xb, acc0);
                    else vq_dot_lds(a0, xr + g, d, acc0);
                    const int code0 = ct * 16 + 4 * g;
                    vq_take_min(acc0, xx, enc + code0, k0 + code0, best, bi);
                    if (sg) {
                        stage_store(cbn, rowsn, pos);
                        pos += STG;
                    }
                }
            }
            // what the MFMA steps did not cover (short chunks, waves without a tile)
            for (; pos < cnt; pos += STG) {
                stage_load(srcn, rowsn, pos);
                stage_store(cbn, rowsn, pos);
            }
#pragma unroll
            for (int i = 0; i < NEN; ++i) {
                const int e = i * nthr + tid;
                if (restage && e < rowsn) enn[e] = sn[i];
            }

            if (c == nch - 1) {   // the head's last chunk: first minimum over the four lane groups, then the epilogue
                vq_merge_groups(best, bi);
                if (g == 0 && row_ok) ind[(size_t)n * H + h] = (int64_t)bi;
                const float* qrow = embed_t + ((size_t)h * K + bi) * d;          // winner row from global memory (L2)
                if constexpr (REG) {
#pragma unroll
                    for (int t = 0; t < NX; ++t) {
                        f32x4 q4 = {0.f, 0.f, 0.f, 0.f};
                        if (row_ok) q4 = *(const f32x4*)(qrow + 16 * t + 4 * g);
                        f32x4 o4, s4, p4 = {0.f, 0.f, 0.f, 0.f};
                        float* dp = diff + (size_t)n * d + 16 * t + 4 * g;      // (DREG false: read and written by this lane alone)
                        if constexpr (DREG) p4 = dacc[t];
                        else if (h > 0 && row_ok) p4 = *(const f32x4*)dp;
                        vq_st_piece(q4, xb[t], p4, h == 0, o4, s4);
                        if constexpr (DREG) {
                            dacc[t] = s4;
                        } else {
                            if (h == H - 1) vq_div_heads(s4, H);
                            if (row_ok) *(f32x4*)dp = s4;
                        }
                        if (row_ok) *(f32x4*)(quant + (size_t)n * D + h * d + 16 * t + 4 * g) = o4;
                    }
                } else {
                    // this lane owns the 16-byte pieces g, g + 4, ... of its frame; the per-head sum of squares lives in diff
                    // itself (read and written by this lane alone), divided by H with the last head
                    if (row_ok)
                        for (int c4 = g; c4 < dv; c4 += 4) {
                            const f32x4 q4 = *(const f32x4*)(qrow + 4 * c4);
                            const f32x4 x4 = *(const f32x4*)(xr + 4 * c4);
                            float* dp = diff + (size_t)n * d + 4 * c4;
                            f32x4 p4 = {0.f, 0.f, 0.f, 0.f}, s4, o4;
                            if (h > 0) p4 = *(const f32x4*)dp;
                            vq_st_piece(q4, x4, p4, h == 0, o4, s4);
                            if (h == H - 1) vq_div_heads(s4, H);
                            *(f32x4*)dp = s4;
                            *(f32x4*)(quant + (size_t)n * D + h * d + 4 * c4) = o4;
                        }
                    wave_sync();             // the next head overwrites the tile slice other lanes just read
                }
            }
            if (restage) {
                __syncthreads();             // chunk q + 1 is complete, and nobody reads chunk q any more
                buf ^= 1;
            }
        }
        if constexpr (DREG) {
            if (row_ok) {
#pragma unroll
                for (int t = 0; t < NX; ++t) {
                    f32x4 v = dacc[t];
                    vq_div_heads(v, H);
                    *(f32x4*)(diff + (size_t)n * d + 16 * t + 4 * g) = v;
                }
            }
        }
    }
}

typedef void (*vq_search_stream_fn)(const float*, const float*, const float*, float*, float*, int64_t*, int, int, int, int,
                                    int, int);

// LDS bytes of the two chunk buffers (rows at pitch d + 4, norms)
static inline size_t vqst_chunk_bytes(int d, int Kc) { return (size_t)2 * Kc * (d + 5) * sizeof(float); }

// chunk = 0: the launcher's choice; chunk > 0 (a multiple of 16, at most VQS_MAX_CHUNK): forced.  `reg`: the register family
// where d allows (the family msmc_vq_search would take for this d), else the LDS-tile family.
static int vq_stream_launch(const float* x, const float* embed_t, const float* enorm, float* quant, float* diff,
                            int64_t* ind, int N, int D, int H, int K, int chunk, bool reg, msmc_stream stream) {
    const int d = D / H;
    if (chunk < 0 || chunk % 16 || chunk > VQS_MAX_CHUNK) return MSMC_E_SHAPE;
    if ((double)N * D * 4.0 >= 4294967296.0) return MSMC_E_SHAPE;     // (32-bit frame byte offsets, as the shortlist launcher)
    vq_search_stream_fn fn = nullptr;
    if (reg && d % 16 == 0) fn = VQ_BY_D4H(vq_search_stream_kernel, d / 16);
    const bool lds_tile = !fn;
    if (lds_tile) fn = vq_search_stream_kernel<0>;
    // LDS-tile family: the widest workgroup whose tile slices leave room for two 16-codeword buffers
    int nw = 4;
    size_t xt = 0;
    if (lds_tile) {
        for (;; nw >>= 1) {
            xt = (size_t)nw * VQ_TILE * (d + 4) * sizeof(float);
            if (xt + vqst_chunk_bytes(d, 16) <= VQ_LDS_LIMIT) break;
            if (nw == 1) return MSMC_E_SHAPE;
        }
    }
    int Kc = chunk;
    if (Kc == 0) {
        // the largest chunk that keeps the workgroup at or under 80 KiB (two per CU); where not even 16 codewords do, 160 KiB
        const size_t room = xt + vqst_chunk_bytes(d, 16) <= 80 * 1024 ? 80 * 1024 : VQ_LDS_LIMIT;
        Kc = (int)((room - xt) / vqst_chunk_bytes(d, 16)) * 16;
        if (Kc > VQS_MAX_CHUNK) Kc = VQS_MAX_CHUNK;
    }
    if (Kc > K) Kc = K;
    const size_t lds = xt + vqst_chunk_bytes(d, Kc);
    if (lds > VQ_LDS_LIMIT) return MSMC_E_SHAPE;
    int rc = msmc_allow_lds((const void*)fn, (int)lds);
    if (rc) return rc;
    const int grid = vq_grid(N, nw, (lds <= 80 * 1024 ? 2 : 1) * MSMC_NUM_CU);
    MSMC_LAUNCH(fn, dim3(grid), dim3(64 * nw), lds, (msmc_stream_t)stream, x, embed_t, enorm, quant, diff, ind, N, D, H, K,
                Kc, (int)vqst_chunk_bytes(d, Kc));
    msmc_vq_last = msmc_prof_name("vq_search_stream_kernel");
    return msmc_check_launch();
}
