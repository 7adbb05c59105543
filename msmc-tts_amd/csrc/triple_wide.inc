// triple_wide.inc -- triple (hinge) loss against ONE wide head (k-means unit codebooks: d = 768 / 1024, any K) (included from
// losses.hip).
//
// Same expressions as triple_loss_kernel of losses.hip with H = 1.  The resident and streamed kernels keep a frame's d channels
// and its running sum of active codewords in registers: at d = 1024 neither fits.  Here both halves of the work are GEMMs on
// v_mfma_f32_16x16x4_f32 (exact fp32), in two launches with a bit mask of the active codewords between them:
//
// 1. triple_loss_wide_kernel: the K products p.e_k of a frame tile on the slice pipeline of wide_tile.inc (tiling, LDS buffers,
//    hand-over, MFMA step and channel order: there), the pipeline of vq_search_wide_kernel (vq_wide.inc).  A wave owns
//    16 frames x the whole centroid tile of 64; NW = 1 / 2 / 4 waves make a workgroup (the launcher picks NW from
//    N: few frames still fill the CUs).  |p|^2 and pos = sum_c (p_c - e_trg,c)^2 come from global memory before the loop, lane
//    group g of a frame taking the 16-byte pieces g, g + 4, ...  After a tile's last slice lane (f, g) holds the products of
//    frame f with codewords 64 kt + 16 m + 4 g + r: t_k = pos - ((|p|^2 - 2 p.e_k) + |e_k|^2), active when t_k != 0 and
//    t_k + margin > 0; the active t_k + margin add up per lane (tiles, m, r ascending), the four lane groups by the butterfly
//    (16, then 32), and lossh = that sum times 1 / d (or 1 / (d K)), one factor rounded once by the host.  The lane's 16
//    decisions -- the target's own bit cleared, whatever its t_k rounds to -- go to mask[n][kt][g] (16 bits, bit 4 m + r).
// 2. triple_grad_wide_kernel: gp = scale (2 / d) (mask x embed_t - n_active e_trg) per (frame tile, window of 128 channels).
//    The rows of a centroid tile (64 x 128 floats at a pitch of 132) pass
//    through two LDS buffers as above; lane (f, g) feeds bit 4 m + r of its mask field as 0.f / 1.f (exact) against row
//    16 m + 4 g + r, so every output element is a chain over the tile's 64 codewords in the order (m, r, g).  One 16-byte LDS
//    read of a row feeds four matrix instructions: an accumulator holds every fourth channel of a 64-channel block.  The tile
//    sums enter a compensated (Kahan) sum over the tiles, n_active is the population count of the mask, and the result is
//    gscale (fma(-n_active, e_trg, s) - compensation).  WF = 2 / 4 of the four waves split the frames, the others the
//    channel window.
//
// Order of arithmetic: fixed by (d, K) alone -- never by N, NW / WF, the grid or the other frames of a tile.  No atomics; every
// global store is a vector-memory store.

// (a centroid tile of both passes is WIDE_KT = 64 codewords: the bits of a mask word)
#define TRW_DC 128                   // channels per window (pass 2)
#define TRW_EPITCH (TRW_DC + 4)      // floats per row of a window buffer

// tests / tools (include/msmc_hip_debug.h): frames per workgroup of both launches, 16 / 32 / 64; 0 = the launcher's choice
static int triple_wide_frames = 0;
extern "C" void msmc_triple_wide_set_frames(int ft) { triple_wide_frames = ft; }

template <int NW>
__global__ __launch_bounds__(64 * NW) void triple_loss_wide_kernel(const float* __restrict__ p, const long long* __restrict__ trg,
                                                                   const float* __restrict__ embed_t,
                                                                   const float* __restrict__ enorm, float* __restrict__ lossh,
                                                                   unsigned short* __restrict__ mask, int N, int d, int K,
                                                                   float margin, float lscale) {
    MSMC_DYN_LDS(smem);
    constexpr int NTHR = 64 * NW, FT = 16 * NW, KT = WIDE_KT, ROWS = FT + KT;
    float* sl = (float*)smem;                                         // [2][ROWS][WIDE_PITCH]: frame rows, then centroid rows
    float* en = sl + 2 * ROWS * WIDE_PITCH;                           // [2][KT]
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int f = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * FT;
    const int nds = (d + WIDE_DS - 1) / WIDE_DS;
    const int nkt = (K + KT - 1) / KT;
    const int total = nkt * nds;
    const int n = n0 + 16 * w + f;
    const bool ok = n < N;                                            // (lanes past the last frame compute on frame N-1 and
    const int nl = ok ? n : N - 1;                                    //  store nothing)

    WideStage<FT, KT, NTHR> stage;                                    // (NTHR >= KT: one norm per work-item; 0.f past K)
    stage.load(p, n0, N, embed_t, 0, K, d, 0, tid);
    stage.store(sl, d, 0, tid);
    wide_norm_store(en, 0, KT, tid, wide_norm_fetch(enorm, 0, KT, K, tid, 0.f));

    // |p|^2 and the direct squared difference to the target's row (global memory / L2): lane group g takes pieces g, g + 4, ...
    long long t = trg[nl];
    t = t < 0 ? 0 : (t >= K ? K - 1 : t);
    float pp = 0.f, pos = 0.f;
    {
        const float* xr = p + (size_t)nl * d;
        const float* er = embed_t + (size_t)t * d;
        for (int c = 4 * g; c < d; c += 16) {
            const f32x4 x4 = *(const f32x4*)(xr + c);
            const f32x4 e4 = *(const f32x4*)(er + c);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float sq = x4[i] * x4[i];
                pp = pp + sq;
                const float df = x4[i] - e4[i];
                const float dq = df * df;
                pos = pos + dq;
            }
        }
        pp = pp + wave_xor16(pp);
        pp = pp + wave_xor32(pp);
        pos = pos + wave_xor16(pos);
        pos = pos + wave_xor32(pos);
    }
    __syncthreads();

    int buf = 0;
    float lsum = 0.f;
    f32x4 acc[4];
    for (int q = 0; q < total; ++q) {
        const int kt = q / nds, s = q - kt * nds;
        const bool more = q + 1 < total;
        const bool next_tile = more && s + 1 == nds;
        const int kt1 = next_tile ? kt + 1 : kt, s1 = next_tile ? 0 : s + 1;      // slice q + 1
        float nn = 0.f;
        if (more) stage.load(p, n0, N, embed_t, kt1 * KT, K, d, s1 * WIDE_DS, tid);
        if (next_tile) nn = wide_norm_fetch(enorm, kt1, KT, K, tid, 0.f);
        if (s == 0) {
#pragma unroll
            for (int m = 0; m < 4; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const float* slc = sl + buf * ROWS * WIDE_PITCH;
        wide_slice_mfma(slc + (16 * w + f) * WIDE_PITCH + 4 * g, slc + (FT + f) * WIDE_PITCH + 4 * g, wide_groups(d, s * WIDE_DS),
                        acc, [](const f32x4&) {});
        if (more) stage.store(sl + (buf ^ 1) * ROWS * WIDE_PITCH, d, s1 * WIDE_DS, tid);
        if (next_tile) wide_norm_store(en, kt1, KT, tid, nn);

        if (s == nds - 1) {   // the tile's last slice: the hinge decisions of this lane's 16 codewords
            const float* enc = wide_norm_tile(en, kt, KT) + 4 * g;
            const int k0 = kt * KT + 4 * g;
            unsigned int bits = 0u;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const f32x4 e4 = *(const f32x4*)(enc + 16 * m);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int k = k0 + 16 * m + r;
                    const float t2 = 2.f * acc[m][r];
                    const float dist = (pp - t2) + e4[r];
                    const float tr = pos - dist;
                    const float v = tr + margin;
                    const bool act = k < K && tr != 0.f && v > 0.f;
                    if (act) lsum = lsum + v;
                    if (act && k != (int)t) bits |= 1u << (4 * m + r);
                }
            }
            if (ok) mask[((size_t)n * nkt + kt) * 4 + g] = (unsigned short)bits;
        }
        __syncthreads();         // slice q + 1 is complete, and nobody reads slice q (or this tile's norms) any more
        buf ^= 1;
    }
    lsum = lsum + wave_xor16(lsum);
    lsum = lsum + wave_xor32(lsum);
    if (ok && g == 0) lossh[n] = lsum * lscale;
}

template <int WF>
__global__ __launch_bounds__(256) void triple_grad_wide_kernel(const long long* __restrict__ trg, const float* __restrict__ embed_t,
                                                              const unsigned short* __restrict__ mask, float* __restrict__ gp,
                                                              int N, int d, int K, float gscale) {
    MSMC_DYN_LDS(smem);
    constexpr int WCH = 4 / WF, FT = 16 * WF, CW = TRW_DC / WCH, NB = CW / 64;
    constexpr int NST = WIDE_KT * (TRW_DC / 4) / 256;                 // 16-byte pieces per work-item per tile
    float* eb = (float*)smem;                                         // [2][WIDE_KT][TRW_EPITCH]
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int f = lane & 15, g = lane >> 4;
    const int wf = w / WCH, wc = w - wf * WCH;
    const int n = blockIdx.x * FT + 16 * wf + f;
    const bool ok = n < N;
    const int c0 = blockIdx.y * TRW_DC;
    const int cw = d - c0 < TRW_DC ? d - c0 : TRW_DC;                 // channels of this window (a multiple of 16)
    const int nkt = (K + WIDE_KT - 1) / WIDE_KT;

    f32x4 st[NST];
    auto stage_load = [&](int kt) {                                   // (zeros past K and past the window: they are multiplied)
#pragma unroll
        for (int i = 0; i < NST; ++i) {
            const int e = i * 256 + tid;
            st[i] = wide_piece(embed_t, kt * WIDE_KT + (e >> 5), K, d, c0 + 4 * (e & 31), c0 + cw);
        }
    };
    auto stage_store = [&](float* dst) {
#pragma unroll
        for (int i = 0; i < NST; ++i) {
            const int e = i * 256 + tid;
            *(f32x4*)(dst + (e >> 5) * TRW_EPITCH + 4 * (e & 31)) = st[i];
        }
    };
    auto mask_of = [&](int kt) { return ok ? (unsigned int)mask[((size_t)n * nkt + kt) * 4 + g] : 0u; };

    stage_load(0);
    stage_store(eb);
    unsigned int h = mask_of(0);
    __syncthreads();

    // accumulator (blk, i) holds the channels 64 blk + 4 x + i, x = 0 .. 15, of the wave's part of the window: one 16-byte read
    // of a row feeds four matrix instructions, and element r of the four accumulators i = 0 .. 3 is one 16-byte piece of gp
    f32x4 acc[4 * NB], s[4 * NB], sc[4 * NB];
#pragma unroll
    for (int a = 0; a < 4 * NB; ++a) s[a] = sc[a] = f32x4{0.f, 0.f, 0.f, 0.f};
    int cnt = 0, buf = 0;
    for (int kt = 0; kt < nkt; ++kt) {
        const bool more = kt + 1 < nkt;
        unsigned int hn = 0u;
        if (more) {
            stage_load(kt + 1);
            hn = mask_of(kt + 1);
        }
#pragma unroll
        for (int a = 0; a < 4 * NB; ++a) acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float* ebc = eb + buf * WIDE_KT * TRW_EPITCH + 4 * g * TRW_EPITCH + wc * CW + 4 * f;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float b = (float)((h >> j) & 1u);
            const float* row = ebc + (16 * (j >> 2) + (j & 3)) * TRW_EPITCH;
#pragma unroll
            for (int blk = 0; blk < NB; ++blk) {
                const f32x4 a4 = *(const f32x4*)(row + 64 * blk);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[4 * blk + i] = mfma_f32_16x16x4(a4[i], b, acc[4 * blk + i]);
            }
        }
        cnt += __builtin_popcount(h);
        // (s, sc) += the tile's sum, Kahan: the exact sum is s - sc within an ulp of s
#pragma unroll
        for (int a = 0; a < 4 * NB; ++a) {
            const f32x4 y = acc[a] - sc[a];
            const f32x4 tt = s[a] + y;
            sc[a] = (tt - s[a]) - y;
            s[a] = tt;
        }
        if (more) stage_store(eb + (buf ^ 1) * WIDE_KT * TRW_EPITCH);
        h = hn;
        __syncthreads();         // tile kt + 1 is complete, and nobody reads tile kt any more
        buf ^= 1;
    }
    cnt = cnt + wave_xor16(cnt);
    cnt = cnt + wave_xor32(cnt);
    if (!ok) return;
    const float nact = (float)cnt;
    long long t = trg[n];
    t = t < 0 ? 0 : (t >= K ? K - 1 : t);
    const float* et = embed_t + (size_t)t * d + c0;                   // the target's row from global memory (L2)
    float* gpp = gp + (size_t)n * d + c0;
#pragma unroll
    for (int blk = 0; blk < NB; ++blk) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = wc * CW + 64 * blk + 16 * g + 4 * r;        // row 4 g + r of the accumulators -> channels c .. c + 3
            if (c < cw) {
                const f32x4 e = *(const f32x4*)(et + c);
                f32x4 g4;
#pragma unroll
                for (int i = 0; i < 4; ++i) g4[i] = gscale * (fmaf(-nact, e[i], s[4 * blk + i][r]) - sc[4 * blk + i][r]);
                *(f32x4*)(gpp + c) = g4;
            }
        }
    }
}

typedef void (*triple_loss_wide_fn)(const float*, const long long*, const float*, const float*, float*, unsigned short*, int, int,
                                    int, float, float);
typedef void (*triple_grad_wide_fn)(const long long*, const float*, const unsigned short*, float*, int, int, int, float);

// the mask: a 64-bit word per (frame, centroid tile)
static inline size_t trw_workspace_bytes(int N, int K) { return (size_t)N * ((K + WIDE_KT - 1) / WIDE_KT) * 8; }

static int triple_wide_launch(const float* p, const int64_t* trg, const float* embed_t, const float* enorm, float* lossh, float* gp,
                              int N, int d, int K, float margin, int mean, void* workspace, size_t workspace_bytes,
                              msmc_stream stream) {
    if (N < 0 || !wide_takes(d, K)) return MSMC_E_SHAPE;
    if (N == 0) return 0;
    if (!workspace || workspace_bytes < trw_workspace_bytes(N, K)) return MSMC_E_WORKSPACE;
    // frames per workgroup: 64 once such workgroups fill every CU, fewer while they would not
    int ft = triple_wide_frames;
    if (ft != 16 && ft != 32 && ft != 64) ft = (N + 63) / 64 >= MSMC_NUM_CU ? 64 : ((N + 31) / 32 >= MSMC_NUM_CU ? 32 : 16);
    const int nw = ft / 16;
    const int ft2 = ft == 64 ? 64 : 32;                              // (the second launch has d / 128 workgroups per frame tile)
    triple_loss_wide_fn f1 = nw == 4 ? triple_loss_wide_kernel<4> : nw == 2 ? triple_loss_wide_kernel<2> : triple_loss_wide_kernel<1>;
    triple_grad_wide_fn f2 = ft2 == 64 ? triple_grad_wide_kernel<4> : triple_grad_wide_kernel<2>;
    const size_t lds1 = wide_lds_floats(ft, WIDE_KT) * sizeof(float);
    const size_t lds2 = (size_t)2 * WIDE_KT * TRW_EPITCH * sizeof(float);
    int rc = msmc_allow_lds((const void*)f1, (int)lds1);
    if (rc) return rc;
    rc = msmc_allow_lds((const void*)f2, (int)lds2);
    if (rc) return rc;
    // the two output factors, each rounded once: 1 / d and 2 / d are exact where d is a power of two, and with the mean where
    // K is one too
    const double kd = (double)d * (mean ? (double)K : 1.0);
    const unsigned gx = (unsigned)((N + ft - 1) / ft);
    MSMC_LAUNCH(f1, dim3(gx), dim3(64 * nw), lds1, (msmc_stream_t)stream, p, (const long long*)trg, embed_t, enorm, lossh,
                (unsigned short*)workspace, N, d, K, margin, (float)(1.0 / kd));
    msmc_loss_last = msmc_prof_name("triple_loss_wide_kernel");
    rc = msmc_check_launch();
    if (rc) return rc;
    MSMC_LAUNCH(f2, dim3((unsigned)((N + ft2 - 1) / ft2), (unsigned)((d + TRW_DC - 1) / TRW_DC)), dim3(256), lds2, (msmc_stream_t)stream, (const long long*)trg,
                embed_t, (const unsigned short*)workspace, gp, N, d, K, (float)(2.0 / kd));
    msmc_prof_name("triple_grad_wide_kernel");
    return msmc_check_launch();
}
