// triple_stream.inc -- triple (hinge) loss against codebooks that do not fit LDS (included from losses.hip).
//
// Same contract as triple_loss_kernel of losses.hip (msmc_triple_loss): lossh [N][H] and gp [N][H d] by the expressions there.
// One head's codebook is never resident: it passes through LDS in chunks of Kc codewords -- rows [Kc][d] plus the Kc squared
// norms -- in two buffers.  While the workgroup consumes chunk q from one buffer, the rows of chunk q + 1 travel HBM / L2 ->
// registers (loads issued ahead of a group of codewords) -> the other buffer (stores behind that group); one workgroup barrier
// per chunk closes the hand-over.  The last chunk is ragged when K % Kc != 0.  A workgroup keeps its frames (blockDim.x / L of
// one head, blockIdx.y) for the whole pass over K.
//
// Registers: a frame's d channels are split over L lanes of its wave (L = 1 wherever the resident kernel takes the head shape
// and for d <= 64; L = 4 for d = 128 beyond LDS, 8 for d = 256 / 512), lane part j holding the 16-byte pieces c L + j of the
// prediction x and of the running sum s of active codewords: 32 or 64 registers each instead of 2 x 256 / 2 x 512.  The L lanes of a frame read L contiguous pieces of a codeword row and all frames
// read the same row (LDS broadcast; no bank conflicts at pitch d).  Per codeword each lane forms its partial dot product, the L
// partials are added by an xor butterfly (masks 16, 32, then 1: a + b and b + a are the same fp32 number, so the L lanes hold the
// same bits and take the same hinge decision), and every lane carries loss and the active count redundantly.
//
// Order of arithmetic: fixed by (d, K) alone -- never by Kc, the workgroup width or the grid.  Codewords enter loss, the active
// count and s in ascending k across chunks.  L = 1: channels 0 .. d-1 in one chain, unfused multiply and add, i.e. the resident
// kernel's order and bits (s += a e with a in {0, 1} is exact in the product, so the fused form here rounds as the unfused one
// there).  L > 1 (no resident kernel defines the bits): four fused chains per lane (vector element i of the pieces, pieces in
// ascending order), (c0 + c1) + (c2 + c3), then the butterfly; the active rows add up in blocks of 8 codewords (by index in K),
// the block sums in a compensated (Kahan) sum, and the gradient is fma(-n_active, e_trg, s) minus the compensation: the
// accumulation over up to K rows costs the roundings of 8 small terms plus an ulp of the result, not K ulps of a large sum.
// No atomics; every global store is a vector-memory store.

#define TRS_LDS_LIMIT ((size_t)160 * 1024)
#define TRS_STG 2                    // 16-byte pieces per work-item staged per group of codewords

MSMC_DEV f32x4 trs_fma4(f32x4 a, f32x4 b, f32x4 c) {
    f32x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = fmaf(a[i], b[i], c[i]);
    return r;
}

// sum over the L lanes that share a frame, the same bits in each of them (a + b and b + a are one fp32 number)
template <int L>
MSMC_DEV float trs_lane_sum(float v) {
    if (L >= 4) {
        v = v + wave_xor16(v);
        v = v + wave_xor32(v);
    }
    if (L == 8) v = v + wave_xor(v, 1);
    return v;
}

template <int D4L, int L>
__global__ __launch_bounds__(256, (L == 1 ? D4L <= 16 : D4L <= 8) ? 2 : 1) void triple_loss_stream_kernel(
    const float* __restrict__ p, const long long* __restrict__ trg, const float* __restrict__ embed_t,
    const float* __restrict__ enorm, float* __restrict__ lossh, float* __restrict__ gp, int N, int H, int K, int Kc,
    float margin, int mean) {
    MSMC_DYN_LDS(smem);
    constexpr int d = 4 * D4L * L, dv = D4L * L;
    float* cb = (float*)smem;                           // [2][Kc][d]
    float* en = cb + (size_t)2 * Kc * d;                // [2][Kc]
    const int nthr = blockDim.x, tid = threadIdx.x, h = blockIdx.y;
    // lane -> (frame of the wave, channel part j): the parts of a frame sit 16 / 32 lanes apart, where the butterfly is the
    // row / half swap (vector ALU, no LDS round trip); the third bit of L = 8 is lane bit 0
    const int lane = tid & 63;
    const int j = L == 1 ? 0 : ((lane >> 4) | (L == 8 ? (lane & 1) << 2 : 0));
    const int fiw = L == 1 ? lane : (L == 4 ? (lane & 15) : (lane & 15) >> 1);
    const int n = blockIdx.x * (nthr / L) + (tid >> 6) * (64 / L) + fiw;
    const bool ok = n < N;                              // (lanes past the last frame compute on frame N-1 and store nothing:
    const int nl = ok ? n : N - 1;                      //  every lane reaches every barrier and every butterfly)
    const int D = H * d;
    const float* eh = embed_t + (size_t)h * K * d;
    const float* nh = enorm + (size_t)h * K;
    const int nch = (K + Kc - 1) / Kc;

    f32x4 st[TRS_STG];
    auto stage_load = [&](const float* src, int rows, int pos) {
#pragma unroll
        for (int i = 0; i < TRS_STG; ++i) {
            const int e = (pos + i) * nthr + tid;
            if (e < rows * dv) st[i] = ((const f32x4*)src)[e];
        }
    };
    auto stage_store = [&](float* dst, int rows, int pos) {
#pragma unroll
        for (int i = 0; i < TRS_STG; ++i) {
            const int e = (pos + i) * nthr + tid;
            if (e < rows * dv) ((f32x4*)dst)[e] = st[i];
        }
    };

    {   // chunk 0 -> buffer 0
        const int rows = Kc < K ? Kc : K;
        const int cnt = (rows * dv + nthr - 1) / nthr;
        for (int pos = 0; pos < cnt; pos += TRS_STG) {
            stage_load(eh, rows, pos);
            stage_store(cb, rows, pos);
        }
        for (int e = tid; e < rows; e += nthr) en[e] = nh[e];
    }

    f32x4 x[D4L], s[D4L], sc[L == 1 ? 1 : D4L], sb[L == 1 ? 1 : D4L];
    auto flush = [&]() {                                // (s, sc) += sb, Kahan: the exact sum is s - sc within an ulp of s
#pragma unroll
        for (int c = 0; c < (L == 1 ? 1 : D4L); ++c) {
            const f32x4 y = sb[c] - sc[c];
            const f32x4 t = s[c] + y;
            sc[c] = (t - s[c]) - y;
            s[c] = t;
            sb[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    float pp = 0.f;
    const float* xp = p + (size_t)nl * D + h * d + 4 * j;
#pragma unroll
    for (int c = 0; c < D4L; ++c) {
        x[c] = *(const f32x4*)(xp + 4 * L * c);
        s[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (L > 1) sc[c] = sb[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i) pp = pp + x[c][i] * x[c][i];
    }
    long long t = trg[(size_t)nl * H + h];
    t = t < 0 ? 0 : (t >= K ? K - 1 : t);
    const float* et = eh + (size_t)t * d + 4 * j;       // the target's row from global memory (L2)
    float pos_d = 0.f;
#pragma unroll
    for (int c = 0; c < D4L; ++c) {
        const f32x4 e = *(const f32x4*)(et + 4 * L * c);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float df = x[c][i] - e[i];
            pos_d = pos_d + df * df;
        }
    }
    pp = trs_lane_sum<L>(pp);
    pos_d = trs_lane_sum<L>(pos_d);
    __syncthreads();

    const float invd = 1.f / (float)d;
    float loss = 0.f, nact = 0.f;
    int buf = 0;
    for (int q = 0; q < nch; ++q) {
        const int k0 = q * Kc;
        const int rows = K - k0 < Kc ? K - k0 : Kc;
        const bool restage = q + 1 < nch;
        const int k0n = k0 + Kc;
        const int rowsn = restage ? (K - k0n < Kc ? K - k0n : Kc) : 0;
        const float* srcn = eh + (size_t)k0n * d;
        const float* cbc = cb + (size_t)buf * Kc * d;
        const float* enc = en + buf * Kc;
        float* cbn = cb + (size_t)(buf ^ 1) * Kc * d;
        float* enn = en + (buf ^ 1) * Kc;
        const int cnt = (rowsn * dv + nthr - 1) / nthr;
        const float sn = tid < rowsn ? nh[k0n + tid] : 0.f;
        // codewords per staging step: the group whose rows make TRS_STG pieces per work-item
        int kq = TRS_STG * nthr / dv;
        kq = kq < 1 ? 1 : kq;
        int pos = 0;
        for (int kb = 0; kb < rows; kb += kq) {
            const bool sg = pos < cnt;
            if (sg) stage_load(srcn, rowsn, pos);
            const int ke = kb + kq < rows ? kb + kq : rows;
            for (int k = kb; k < ke; ++k) {
                const float* ek = cbc + (size_t)k * d + 4 * j;
                f32x4 e[D4L];
                float dot = 0.f;
                if constexpr (L == 1) {
#pragma unroll
                    for (int c = 0; c < D4L; ++c) {
                        e[c] = *(const f32x4*)(ek + 4 * c);
#pragma unroll
                        for (int i = 0; i < 4; ++i) dot = dot + x[c][i] * e[c][i];
                    }
                } else {
                    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int c = 0; c < D4L; ++c) {
                        e[c] = *(const f32x4*)(ek + 4 * L * c);
                        acc = trs_fma4(x[c], e[c], acc);
                    }
                    dot = trs_lane_sum<L>((acc[0] + acc[1]) + (acc[2] + acc[3]));
                }
                const float dist = (pp - 2.f * dot) + enc[k];
                const float tr = pos_d - dist;
                const float v = tr + margin;
                const float a = (tr != 0.f && v > 0.f) ? 1.f : 0.f;
                loss = loss + a * (v * invd);
                nact = nact + a;
                const f32x4 a4 = {a, a, a, a};
                if constexpr (L == 1) {
#pragma unroll
                    for (int c = 0; c < D4L; ++c) s[c] = trs_fma4(a4, e[c], s[c]);
                } else {
                    // two levels: the active rows of codewords 8 m .. 8 m + 7 (m by the codeword's index in K, not in the chunk)
                    // add up in sb, a plain chain of at most 8 small terms; sb then enters the compensated sum (s, sc)
#pragma unroll
                    for (int c = 0; c < D4L; ++c) sb[c] = trs_fma4(a4, e[c], sb[c]);
                    if (((k0 + k) & 7) == 7) flush();
                }
            }
            if (sg) {
                stage_store(cbn, rowsn, pos);
                pos += TRS_STG;
            }
        }
        for (; pos < cnt; pos += TRS_STG) {             // what the groups did not cover
            stage_load(srcn, rowsn, pos);
            stage_store(cbn, rowsn, pos);
        }
        if (tid < rowsn) enn[tid] = sn;
        for (int e = tid + nthr; e < rowsn; e += nthr) enn[e] = nh[k0n + e];
        if (restage) {
            __syncthreads();                            // chunk q + 1 is complete, and nobody reads chunk q any more
            buf ^= 1;
        }
    }

    if constexpr (L > 1) {
        if (K & 7) flush();                             // the last, short block
    }
    if (!ok) return;
    const float scale = mean ? 1.f / (float)K : 1.f;
    if (j == 0) lossh[(size_t)n * H + h] = loss * scale;
    const float gs = 2.f * invd * scale;
    float* gpp = gp + (size_t)n * D + h * d + 4 * j;
#pragma unroll
    for (int c = 0; c < D4L; ++c) {
        const f32x4 e = *(const f32x4*)(et + 4 * L * c);
        f32x4 g4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if constexpr (L == 1) g4[i] = gs * (s[c][i] - nact * e[i]);
            else g4[i] = gs * (fmaf(-nact, e[i], s[c][i]) - sc[c][i]);
        }
        *(f32x4*)(gpp + 4 * L * c) = g4;
    }
}

typedef void (*triple_stream_fn)(const float*, const long long*, const float*, const float*, float*, float*, int, int, int, int,
                                 float, int);

// LDS bytes of the two chunk buffers (rows at pitch d, norms)
static inline size_t trs_chunk_bytes(int d, int Kc) { return (size_t)2 * Kc * (d + 1) * sizeof(float); }

// chunk = 0: the launcher's choice; chunk > 0: forced (larger than K means K)
static int triple_stream_launch(const float* p, const int64_t* trg, const float* embed_t, const float* enorm, float* lossh,
                                float* gp, int N, int D, int H, int K, float margin, int mean, int chunk, msmc_stream stream) {
    const int d = D / H;
    triple_stream_fn fn;
    int L = 1;
    switch (d) {
        case 16: fn = triple_loss_stream_kernel<4, 1>; break;
        case 32: fn = triple_loss_stream_kernel<8, 1>; break;
        case 64: fn = triple_loss_stream_kernel<16, 1>; break;
        case 128:
            // where the resident kernel takes (K, 128) its bits are the contract: L = 1; beyond LDS there are none to match
            if (((size_t)K * d + K) * sizeof(float) <= TRS_LDS_LIMIT) fn = triple_loss_stream_kernel<32, 1>;
            else { fn = triple_loss_stream_kernel<8, 4>; L = 4; }
            break;
        case 256: fn = triple_loss_stream_kernel<8, 8>; L = 8; break;
        case 512: fn = triple_loss_stream_kernel<16, 8>; L = 8; break;
        default: return MSMC_E_SHAPE;
    }
    if (chunk < 0) return MSMC_E_SHAPE;
    int Kc = chunk;
    if (Kc == 0) {
        // the largest multiple of 8 that keeps a workgroup at or under 80 KiB (two per CU), at most 64 (a short first chunk: its
        // load is the only one nothing hides)
        Kc = (int)((size_t)80 * 1024 / trs_chunk_bytes(d, 8)) * 8;
        if (Kc > 64) Kc = 64;
    }
    if (Kc > K) Kc = K;
    const size_t lds = trs_chunk_bytes(d, Kc);
    if (lds > TRS_LDS_LIMIT) return MSMC_E_SHAPE;
    if (N == 0) return 0;
    // narrower workgroups while the grid would leave CUs idle (every workgroup streams the whole head: wide where N allows)
    int nthr = 256;
    while (nthr > 64 && (long)((N + nthr / L - 1) / (nthr / L)) * H < MSMC_NUM_CU) nthr >>= 1;
    int rc = msmc_allow_lds((const void*)fn, (int)lds);
    if (rc) return rc;
    const dim3 grid((unsigned)((N + nthr / L - 1) / (nthr / L)), (unsigned)H);
    MSMC_LAUNCH(fn, grid, dim3(nthr), lds, (msmc_stream_t)stream, p, (const long long*)trg, embed_t, enorm, lossh, gp, N, H, K, Kc,
                margin, mean);
    msmc_loss_last = msmc_prof_name("triple_loss_stream_kernel");
    return msmc_check_launch();
}
