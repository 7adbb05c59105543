// gather7.inc -- seventh-generation bf16 forward / data-gradient implicit GEMM (variants 56, 59, 60, 61, 63; included by conv.hip after
// gather5.inc, whose descriptor semantics, lattice / tap tables, source-swizzled LDS-DMA images and in-register epilogue it keeps).
//
// Reference layers: the k = 3 feed-forward convolutions of the FFT blocks (acoustic_models/transformer.py:330-352), the HifiGAN
// ResBlock / MRF convolutions with C >= 128 (msmctts/networks/hifigan/common.py:21-57), the k x 1 period- and 3 x 3
// resolution-discriminator stacks (msmctts/networks/hifigan/discriminator.py:15-154) and their data gradients.
//
// What the fifth generation is bound by (profiles/r03_gather5_microbench.txt, r04_step_sq_summary.txt, DESIGN.md section 8):
// a wave owns ONE 32 x 32 accumulator, so every MFMA needs two fresh 16-byte fragments (2 KB of LDS reads per MFMA and wave:
// at 256 B/clk the LDS array is exactly as busy as the matrix pipes at their peak -- the two cannot both run), and all sixteen
// waves of the CU meet at ONE barrier per stage, which serialises the fragment-read phase and the MFMA phase of a stage.
// Here:
//   * a wave owns a 64 x 64 block of the tile: 2 x 2 accumulators of v_mfma_f32_32x32x16_bf16, FOUR fragment reads for
//     four MFMAs (half the LDS traffic per flop);
//   * EIGHT waves per workgroup and an LDS footprint of at most 80 KB for the workhorse tiles, so that TWO workgroups share
//     a CU: their barriers are independent, one's fragment / DMA phases run under the other's MFMAs;
//   * the contraction of a stage (64-channel chunk, tap) is split over KG wave groups INSIDE the stage (group k takes the
//     k16-steps 4k/KG ..): tiles of 64 x 128 / 128 x 128 keep eight 64 x 64 waves busy, every group reads the same
//     ring slot; the groups' partial blocks meet in LDS at the end (recursive halving: after log2 KG exchanges every wave
//     owns 4 / KG finished blocks, the additions of a block happen in one fixed tree) and every wave runs a share of the epilogue;
//   * double-buffered super-stages: SPB stages (weight slices of SPB (chunk, tap) pairs) per barrier, the NEXT super-stage's
//     slices and -- one chunk ahead -- halo tile in flight under the current one; one s_waitcnt vmcnt(0) + one LDS-only
//     barrier per super-stage, no counted waits.
// Requirements (cv7_plan refuses the rest): bf16, Cin % 8 == 0 and >= 64 (the pieces of the last 64-channel chunk past Cin are read
// from the zero page, on the weight side and on the halo side: the 600-wide FFT blocks of the predictor), Cout % 8 == 0, at least two
// taps, 0 <= in_slope <= 1.
#define CV7_WAVES 8
// PROBE BUILDS ONLY (tools/r05_clock_probe.sh; never defined by the Makefile): with bit 64 of the diagnostics mask set, d.res2 is
// a buffer of 8 x int64 per workgroup that receives shader-clock stamps of the kernel's phases (+ the hardware id word)
#ifdef CV7_CLOCKS
#define CV7_STAMP(k) do { if ((abl & 64) && tid == 0) ((long long*)d.res2)[(size_t)id * 8 + (k)] = msmc_clock(); } while (0)
#else
#define CV7_STAMP(k) do { } while (0)
#endif

struct Cv7Plan {
    int applies;
    int cfg;
    CvGeom G;
    size_t lds;
    int tilesM, tilesN, blocks;
};
struct Cv7Run {
    int tilesM, tilesN;
};
// Two workgroups of eight waves share a CU where the LDS footprint allows it (estimate in KB from the template arguments: halo
// buffers of BM + 8 pixels): those instantiations are held to 128 vector registers per work-item (4 waves per SIMD), the others get 256.
constexpr int cv7_waves_per_simd(int wm, int wn, int spb) { return 1 + 2 * (8 * wm + 1) + 2 * spb * wn * 8 <= 80 ? 4 : 2; }

// WM x WN waves of 64 x 64 per contraction group, KG groups (WM WN KG = 8), SPB stages per barrier (double-buffered super-stages),
// XV = LDS-DMA instructions per wave and halo-tile chunk (eight pixels each: halo tiles of up to 64 XV pixels).
// Measured and NOT kept (profiles/r05_gather7_probe.md): a ring three super-stages deep with counted waits (the loop of the
// 128 x 128 tile took the same 15.8 k cycles per twelve stages: landing latency is not what the loop waits for) and, on that
// ring, the requests issued at the TAIL of a stage instead of its head (17.7 k: every wave then queues its LDS-DMA issue in
// front of the barrier).  What the loop pays for is the ISSUE of the requests (100-200 cycles per instruction next to the
// other waves' fragment reads) and the barrier: fewer, longer super-stages (SPB = 2, 3) are what moved it (13.1 k).
template <int WM, int WN, int KG, int SPB, int XV>
MSMC_DEV void cv7_body(const msmc_conv_desc& d, const CvGeom& G, const Cv7Run& R, const int id) {
    MSMC_DYN_LDS(smem);
    typedef unsigned short T;
    static_assert(WM * WN * KG == CV7_WAVES && (KG == 1 || KG == 2 || KG == 4), "eight waves of 64 x 64");
    constexpr int BM = 64 * WM, BN = 64 * WN, NT = 64 * CV7_WAVES;
    constexpr int KPG = 4 / KG;                                 // k16-steps of a stage per contraction group
    constexpr int WST = BN * 128;                               // one weight slot: [BN rows][128 B]
    const int npix = G.IH * G.IW, IW = G.IW;
    char* dump = smem;                                          // 1 KB: destination of the pieces past the halo tile
    const int xbytes = (npix * 128 + 1023) & ~1023;
    const int tid = threadIdx.x, w = wave_uniform(tid >> 6), lane = tid & 63, li = lane & 31, g = lane >> 5;
    const int kg = w / (WM * WN), wl = w - kg * (WM * WN);      // contraction group, wave within it
    const int wm_ = wl % WM, wn_ = wl / WM;
    char* xbuf0 = smem + 1024;                                  // two halo buffers ...
    constexpr int RD = 2;                                       // ring depth in super-stages
    char* wring = xbuf0 + 2 * xbytes;                           // ... and 2 SPB weight slots
    // block -> (pixel tile, channel tile): the channel tiles of a pixel tile run on one XCD (blocks go round-robin over 8)
    int tm, tn;
    {
        const int per = 8 * R.tilesN;
        const int grp = id / per, r = id - grp * per;
        tm = grp * 8 + (r & 7);
        tn = r >> 3;
        if (tm >= R.tilesM) return;                             // (padding blocks of the last group)
    }
    int bt = tm;
    const int tx_ = bt % G.tilesX;
    bt /= G.tilesX;
    const int ty_ = bt % G.tilesY;
    const int b = bt / G.tilesY;
    const int co0 = tn * BN;
    const int qy0 = ty_ * G.TH, qx0 = tx_ * G.TW;
    const int iyBase = qy0 * d.isy + d.iy0 + G.dyMin, ixBase = qx0 * d.isx + d.ix0 + G.dxMin;
    const int Cin = d.Cin, Cout = d.Cout;
    const int nchunks = (Cin + 63) >> 6, ntaps = d.ntaps;
    const int tailp = (Cin & 63) >> 3;  // 16-byte pieces of the last chunk that hold channels (0: the chunk is whole); the others read zeros
    const int nst = nchunks * ntaps;
    const int abl = d.split_shift;      // DIAGNOSTICS (0 in production; results are garbage otherwise): 2 no weight stream,
                                        // 4 no halo stream, 8 no epilogue, 32 no per-super-stage barrier
    CV7_STAMP(0);

    const T* xb = (const T*)d.x + (size_t)b * d.Hin * d.Win * Cin;
    // per-tap lane tables (lane t): halo-tile row shift and byte offset of the tap's weight slice
    const int tl = lane < ntaps ? lane : 0;
    const int taprow_v = (d.tap_dy[tl] - G.dyMin) * IW + (d.tap_dx[tl] - G.dxMin);
    const unsigned int tapw_v = (unsigned int)d.tap_w[tl] * (unsigned int)Cout * (unsigned int)Cin * 2u;

    // ---- weight slice of a stage: BN rows of 128 B = WN LDS-DMA instructions of eight rows per wave
    const char* wsrc[WN];
    bool wtail[WN];                                             // this lane's piece of instruction u lies past Cin in the last chunk
#pragma unroll
    for (int u = 0; u < WN; ++u) {
        const int n = w * (8 * WN) + u * 8 + (lane >> 3);
        int co = co0 + n;
        if (co >= Cout) co = Cout - 1;                          // columns past Cout are never stored: any valid row
        const int piece = (lane & 7) ^ ((n >> 1) & 7);
        wsrc[u] = (const char*)d.w + ((size_t)co * Cin + (piece << 3)) * 2;
        wtail[u] = tailp && piece >= tailp;
    }
    int ic = 0, it = 0;                                         // (chunk, tap) of the next weight stage to request
    auto issue_w = [&](int slot) {                              // (past the end: the last stage again, never read)
        const size_t soff = (size_t)wave_read_lane(tapw_v, it) + (size_t)ic * 128;
        char* st = wring + slot * WST + w * (8 * WN * 128);
        const bool last = tailp && ic == nchunks - 1;
#pragma unroll
        for (int u = 0; u < WN; ++u)
            lds_dma16(last && wtail[u] ? (const char*)msmc_cv5_zero_page : wsrc[u] + soff, st + u * 1024);
        if (ic * ntaps + it + 1 < nst) {
            if (++it == ntaps) { it = 0; ++ic; }
        }
    };
    if (!(abl & 2)) {
#pragma unroll
        for (int j = 0; j < (RD - 1) * SPB; ++j) issue_w(j);    // the first RD - 1 super-stages, before anything else
    }

    // halo tile by LDS-DMA: instruction q = w + 8 u covers eight pixels of one chunk; this lane's piece of it is the same
    // for every chunk: source-swizzled address in x, or the zero page for padding pixels / pieces past the tile.  No offset
    // table and no barrier before the first request: every lane works out the source of its own XV pixels (1-D tiles
    // without a division), so the first halo chunk is on its way a few hundred cycles into the kernel.
    const int nxq = (npix + 7) >> 3;
    const char* xsrc[XV];
#pragma unroll
    for (int u = 0; u < XV; ++u) {
        const int pi = (w + CV7_WAVES * u) * 8 + (lane >> 3);
        xsrc[u] = (const char*)msmc_cv5_zero_page;
        if (pi < npix) {
            const int ry = G.IH == 1 ? 0 : pi / IW, rx = pi - ry * IW;
            int iy = iyBase + ry, ix = ixBase + rx;
            bool inside = true;
            if (d.pad_mode == 1) {
                iy = reflect_index(iy, d.Hin);
                ix = reflect_index(ix, d.Win);
            } else {
                inside = (iy >= 0) && (iy < d.Hin) && (ix >= 0) && (ix < d.Win);
            }
            if (inside) xsrc[u] = (const char*)(xb + (size_t)(iy * d.Win + ix) * Cin + ((((lane & 7) ^ ((pi >> 1) & 7))) << 3));
        }
    }
    // (the swizzle key of a halo piece, (pixel >> 1) & 7, is the same for all instructions of a lane: eight waves of eight pixels)
    const bool xtail = tailp && ((lane & 7) ^ ((((w & 1) << 2) + (lane >> 4)) & 7)) >= tailp;
    int xnext = 0;                                              // next halo chunk to request
    auto issue_x = [&]() {                                      // (chunk past the end: the last one again, never read)
        const int cc = xnext < nchunks ? xnext : nchunks - 1;
        char* xbuf = xbuf0 + (xnext & 1) * xbytes;
        const bool last = tailp && cc == nchunks - 1;
#pragma unroll
        for (int u = 0; u < XV; ++u) {
            const int q = w + CV7_WAVES * u;
            lds_dma16(last && xtail ? (const char*)msmc_cv5_zero_page : xsrc[u] + cc * 128, q < nxq ? xbuf + q * 1024 : dump);
        }
        ++xnext;
    };
    if (!(abl & 4)) issue_x();
    CV7_STAMP(1);

    // lattice point of accumulator column (pb, li): halo pixel at tap shift 0 and output pixel (-1: outside the image)
    int arow[2], opix[2];
#pragma unroll
    for (int pb = 0; pb < 2; ++pb) {
        const int m = 64 * wm_ + 32 * pb + li;
        const int mty = G.TH == 1 ? 0 : m / G.TW, mtx = m - mty * G.TW;
        const int qy = qy0 + mty, qx = qx0 + mtx;
        const bool valid = mty < G.TH && qy < d.QH && qx < d.QW;
        arow[pb] = (mty < G.TH) ? (mty * d.isy) * IW + mtx * d.isx : 0;
        opix[pb] = valid ? (d.oy0 + qy * d.osy) * d.Wout + (d.ox0 + qx * d.osx) : -1;
    }
    // weight-fragment addresses inside slot 0 for this group's k16-steps (the slot offset is an immediate of the read)
    const char* wfa[2][KPG];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
        const int n = 64 * wn_ + 32 * cb + li;
#pragma unroll
        for (int i = 0; i < KPG; ++i)
            wfa[cb][i] = wring + n * 128 + (((2 * (kg * KPG + i) + g) ^ ((n >> 1) & 7)) << 4);
    }
    const int kpiece = 2 * kg * KPG + g;                        // 16-byte piece of a halo row for k16-step 0 of this group
    f32x16 acc[2][2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int pb = 0; pb < 2; ++pb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[cb][pb][r] = 0.f;
    const float slope = d.in_slope;

    int sc = 0, st_ = 0, s = 0;                                 // (chunk, tap), flattened index of the stage being computed
    // one stage out of ring slot SLOT: this group's k16-steps, fragments of step i+1 in flight under the MFMAs of step i
    auto stage = [&](auto slot_c) {
        constexpr int SLOT = decltype(slot_c)::value;
        const char* xcur = xbuf0 + (sc & 1) * xbytes;
        const int trow = wave_read_lane(taprow_v, st_);
        const char* xa[2];
        int xkey[2];
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) {
            const int row = arow[pb] + trow;
            xa[pb] = xcur + (row << 7);
            xkey[pb] = (row >> 1) & 7;
        }
        auto read_step = [&](auto i_c, u32x4 (&xf)[2], u32x4 (&wf)[2]) {
            constexpr int I = decltype(i_c)::value;
#pragma unroll
            for (int pb = 0; pb < 2; ++pb) xf[pb] = *(const u32x4*)(xa[pb] + (((kpiece + 2 * I) ^ xkey[pb]) << 4));
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) wf[cb] = *(const u32x4*)(wfa[cb][I] + SLOT * WST);
        };
        auto mma_step = [&](const u32x4 (&xf)[2], const u32x4 (&wf)[2]) {
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int pb = 0; pb < 2; ++pb)
                    acc[cb][pb] = mfma_bf16_32x32x16(__builtin_bit_cast(bf16x8, wf[cb]), __builtin_bit_cast(bf16x8, xf[pb]), acc[cb][pb]);
            sched_fence();
        };
        u32x4 xf0[2], wf0[2], xf1[2], wf1[2];
        read_step(std::integral_constant<int, 0>(), xf0, wf0);
        if constexpr (KPG >= 2) read_step(std::integral_constant<int, 1>(), xf1, wf1);
        sched_fence();
        mma_step(xf0, wf0);
        if constexpr (KPG >= 4) {
            read_step(std::integral_constant<int, 2>(), xf0, wf0);
            sched_fence();
        }
        if constexpr (KPG >= 2) mma_step(xf1, wf1);
        if constexpr (KPG >= 4) {
            read_step(std::integral_constant<int, 3>(), xf1, wf1);
            sched_fence();
            mma_step(xf0, wf0);
            mma_step(xf1, wf1);
        }
        ++s;
        if (++st_ == ntaps) { st_ = 0; ++sc; }
    };
    // One super-stage out of ring position PAR.  On entry everything requested so far must have landed (its own slices, the
    // halo chunks it touches): s_waitcnt vmcnt(0), then one LDS-only barrier (everybody's pieces landed; the slots / halo buffer
    // about to be refilled were last read before it), the requests for the next super-stage and -- when this super-stage STARTS
    // inside chunk c and chunk c + 1 is not on its way yet -- for the halo tile of chunk c + 1 (its buffer was last read by
    // chunk c - 1; cv7_plan admits SPB = 1, 2 and ntaps only: with those the request always precedes the super-stage that reads it).
    auto super_stage = [&](auto par_c) {
        constexpr int PAR = decltype(par_c)::value;
        lds_dma_wait();
        if (!(abl & 32)) block_sync_lds();
#ifdef CV7_CLOCKS
        if (s == 0) CV7_STAMP(2);
#endif
        if (xnext <= sc + 1 && !(abl & 4)) issue_x();
        if (!(abl & 2)) {
#pragma unroll
            for (int j = 0; j < SPB; ++j) issue_w((1 - PAR) * SPB + j);
        }
        if (slope != 1.f) {
            // input activation in place on a landed halo chunk, once: the chunk whose tap 0 lies in this super-stage
            const int cact = st_ == 0 ? sc : sc + 1;
            const int first = st_ == 0 ? s : s + (ntaps - st_);
            if (first < s + SPB && cact < nchunks) {
                char* xc = xbuf0 + (cact & 1) * xbytes;
                for (int e = tid; e < npix * 8; e += NT) {
                    u32x4 v = *(const u32x4*)(xc + e * 16);
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = bf16x2_leaky(v[q], slope);
                    *(u32x4*)(xc + e * 16) = v;
                }
                block_sync_lds();
            }
        }
        stage(std::integral_constant<int, PAR * SPB>());
        if constexpr (SPB >= 2) { if (s < nst) stage(std::integral_constant<int, PAR * SPB + 1>()); }
        if constexpr (SPB >= 3) { if (s < nst) stage(std::integral_constant<int, PAR * SPB + 2>()); }
        if constexpr (SPB >= 4) { if (s < nst) stage(std::integral_constant<int, PAR * SPB + 3>()); }
    };
    while (s < nst) {
        super_stage(std::integral_constant<int, 0>());
        if (s < nst) super_stage(std::integral_constant<int, 1>());
    }
    lds_dma_wait();                                             // (the repeated pieces of the stages past the end)
    CV7_STAMP(3);

    // ---- the groups' partial blocks meet in LDS (recursive halving).  Exchange area: smem + 1024 onwards (halo buffers and
    // ring are dead), [wave][block q][register r][lane] floats: lane-contiguous, conflict-free.
    int pbo = 0, cbo = 0;                                       // owned block(s) after the exchanges
    if constexpr (KG >= 2) {
        float* xch = (float*)(smem + 1024);
        block_sync_lds();                                       // every wave is done with the stages
        {
            const int bit = kg & 1;                             // level 1: partner group kg ^ 1, keep pixel block pb = bit
            float* mine = xch + (size_t)w * (2 * 16 * 64);
            if (bit == 0) {
#pragma unroll
                for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) mine[(cb * 16 + r) * 64 + lane] = acc[cb][1][r];
            } else {
#pragma unroll
                for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        mine[(cb * 16 + r) * 64 + lane] = acc[cb][0][r];
                        acc[cb][0][r] = acc[cb][1][r];
                    }
                opix[0] = opix[1];
            }
            block_sync_lds();
            const float* theirs = xch + (size_t)(w ^ (WM * WN)) * (2 * 16 * 64);
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[cb][0][r] = acc[cb][0][r] + theirs[(cb * 16 + r) * 64 + lane];
            pbo = bit;
        }
        if constexpr (KG == 4) {
            block_sync_lds();                                   // level-1 reads done before the area is written again
            const int bit = kg >> 1;                            // level 2: partner group kg ^ 2, keep channel block cb = bit
            float* mine = xch + (size_t)w * (16 * 64);
            if (bit == 0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) mine[r * 64 + lane] = acc[1][0][r];
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    mine[r * 64 + lane] = acc[0][0][r];
                    acc[0][0][r] = acc[1][0][r];
                }
            }
            block_sync_lds();
            const float* theirs = xch + (size_t)(w ^ (2 * WM * WN)) * (16 * 64);
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[0][0][r] = acc[0][0][r] + theirs[r * 64 + lane];
            cbo = bit;
        }
    }
    (void)pbo;

    CV7_STAMP(4);
    // ---- epilogue in registers: lane (li, g) owns lattice point 64 wm + 32 pb + li and, after the swap, the channel runs
    // co0 + 64 wn + 32 cb + 16 h + 8 g + (0 .. 7), h = 0, 1.  Two passes over the wave's finished blocks: every operand load
    // (mask / residuals / bias) first, then arithmetic and stores -- the stores of one block cannot hold back the loads of the next.
    const T* mask = (const T*)d.mask_src;
    const T* res = (const T*)d.res;
#ifdef CV7_CLOCKS
    const T* res2 = (abl & 64) ? nullptr : (const T*)d.res2;
#else
    const T* res2 = (const T*)d.res2;
#endif
    T* out = (T*)d.out;
    const size_t img = (size_t)b * d.Hout * d.Wout;
    const float mslope = d.mask_slope, odiv = d.out_div, oslope = d.out_slope;
    constexpr int NCB = KG == 4 ? 1 : 2, NPB = KG == 1 ? 2 : 1;   // blocks this wave finishes: acc[0 .. NCB)[0 .. NPB)
    // instantiations held to 128 registers (two workgroups per CU) with two finished blocks per wave take them one at a time
    constexpr int CBS = (cv7_waves_per_simd(WM, WN, SPB) == 4 && NCB * NPB > 1) ? 1 : NCB;
    auto finish = [&](auto cb0_c) {
        constexpr int CB0 = decltype(cb0_c)::value;
        u32x4 mk[NPB][CBS][2], r1[NPB][CBS][2], r2[NPB][CBS][2];
        f32x4 bs[CBS][2][2];
#pragma unroll
        for (int c = 0; c < CBS; ++c)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int n = co0 + 64 * wn_ + 32 * (KG == 4 ? cbo : CB0 + c) + 16 * h + 8 * g;
                bs[c][h][0] = bs[c][h][1] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (d.bias && n < Cout) {
                    bs[c][h][0] = *(const f32x4*)(d.bias + n);
                    bs[c][h][1] = *(const f32x4*)(d.bias + n + 4);
                }
            }
#pragma unroll
        for (int pb = 0; pb < NPB; ++pb)
#pragma unroll
            for (int c = 0; c < CBS; ++c)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int po = opix[pb];
                    const int n = co0 + 64 * wn_ + 32 * (KG == 4 ? cbo : CB0 + c) + 16 * h + 8 * g;
                    mk[pb][c][h] = r1[pb][c][h] = r2[pb][c][h] = u32x4{0u, 0u, 0u, 0u};
                    if (po < 0 || n >= Cout || (abl & 8)) continue;
                    const size_t o = (img + po) * Cout + n;
                    if (mask) mk[pb][c][h] = *(const u32x4*)(mask + o);
                    if (res) r1[pb][c][h] = *(const u32x4*)(res + o);
                    if (res2) r2[pb][c][h] = *(const u32x4*)(res2 + o);
                }
#pragma unroll
        for (int pb = 0; pb < NPB; ++pb) {
            const int po = opix[pb];
#pragma unroll
            for (int c = 0; c < CBS; ++c) {
                cv5_swap_runs(acc[CB0 + c][pb]);
                if (po < 0 || (abl & 8)) continue;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int n = co0 + 64 * wn_ + 32 * (KG == 4 ? cbo : CB0 + c) + 16 * h + 8 * g;
                    if (n >= Cout) continue;                    // (Cout % 8 == 0: a run is all in or all out)
                    const size_t o = (img + po) * Cout + n;
                    float ov[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) ov[j] = acc[CB0 + c][pb][8 * h + j] + (j < 4 ? bs[c][h][0][j & 3] : bs[c][h][1][j & 3]);
                    {
                        const u32x4 m_ = mk[pb][c][h], a_ = r1[pb][c][h], b_ = r2[pb][c][h];
                        const unsigned int mkw[4] = {m_[0], m_[1], m_[2], m_[3]}, r1w[4] = {a_[0], a_[1], a_[2], a_[3]},
                                           r2w[4] = {b_[0], b_[1], b_[2], b_[3]};
                        cv_ep<8>(ov, mkw, r1w, r2w, mask != nullptr, res != nullptr, res2 != nullptr, mslope, odiv, oslope);
                    }
                    const u32x4 pk = {pack_bf16x2(ov[0], ov[1]), pack_bf16x2(ov[2], ov[3]), pack_bf16x2(ov[4], ov[5]), pack_bf16x2(ov[6], ov[7])};
                    *(u32x4*)(out + o) = pk;
                }
            }
        }
    };
    finish(std::integral_constant<int, 0>());
    if constexpr (CBS < NCB) finish(std::integral_constant<int, 1>());
#ifdef CV7_CLOCKS
    if (abl & 64) {
        lds_dma_wait();                                         // (stores retired: the stamp below is the end of the workgroup's traffic)
        block_sync_lds();
    }
    CV7_STAMP(5);
#endif
}

template <int WM, int WN, int KG, int SPB, int XV>
__global__ __launch_bounds__(512, cv7_waves_per_simd(WM, WN, SPB)) void conv_gather7_kernel(msmc_conv_desc d, CvGeom G, Cv7Run R) {
    cv7_body<WM, WN, KG, SPB, XV>(d, G, R, (int)blockIdx.x);
}
struct Cv7GroupArgs {
    CvGroupArgs a;
    Cv7Run R[MSMC_GROUP_MAX];
};
template <int WM, int WN, int KG, int SPB, int XV>
__global__ __launch_bounds__(512, cv7_waves_per_simd(WM, WN, SPB)) void conv_gather7_group_kernel(Cv7GroupArgs ga) {
    const int k = cv_group_member(ga.a.first, ga.a.n);
    cv7_body<WM, WN, KG, SPB, XV>(ga.a.d[k], ga.a.G[k], ga.R[k], (int)blockIdx.x - ga.a.first[k]);
}

// variant 56 + cfg; (WM, WN, KG, SPB, XV) -> tile (lattice points x channels), stages per barrier:
//   0: (2, 2, 2, 1, 3) 128 x 128, two workgroups per CU     3: (1, 2, 4, 2, 3)  64 x 128, two stages per barrier
//   4: (4, 2, 1, 2, 5) 256 x 128, two stages per barrier     5: (2, 1, 4, 2, 3) 128 x 64 (64-channel outputs), two per barrier
//   7: (2, 2, 2, 2, 3) 128 x 128, two stages per barrier
// (1, 2, 6 -- 128 x 128 and 64 x 128 with a chunk's three taps per barrier, 128 x 256 -- were timed on every layer of the bench
//  configuration and never chosen: retired, their variant numbers stay unused; profiles/r05_gather7_microbench.txt)
#define CV7_NCFG 8
static bool cv7_is_variant(int variant) {
    return variant == 56 || variant == 59 || variant == 60 || variant == 61 || variant == 63;
}
static void cv7_cfg(int cfg, int* wm, int* wn, int* kg, int* spb, int* xv) {
    static const int T[CV7_NCFG][5] = {{2, 2, 2, 1, 3}, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}, {1, 2, 4, 2, 3},
                                       {4, 2, 1, 2, 5}, {2, 1, 4, 2, 3}, {0, 0, 0, 0, 0}, {2, 2, 2, 2, 3}};
    *wm = T[cfg][0]; *wn = T[cfg][1]; *kg = T[cfg][2]; *spb = T[cfg][3]; *xv = T[cfg][4];
}

static int cv7_plan(const msmc_conv_desc* d, int variant, Cv7Plan* pl) {
    pl->applies = 0;
    if (d->dtype != 1 || !cv7_is_variant(variant)) return 0;
    int wm, wn, kg, spb, xv;
    cv7_cfg(variant - 56, &wm, &wn, &kg, &spb, &xv);
    const int bm = 64 * wm, bn = 64 * wn;
    if (d->Cin % 8 != 0 || d->Cin < 64 || d->Cin > CV5_MAX_CIN || d->Cout % 8 != 0 || d->ntaps < 2 || d->ntaps > MSMC_CONV_MAX_TAPS) return 0;
    if (d->ntaps > 64 || (double)d->ntaps * d->Cout * d->Cin * 2.0 >= 4294967296.0) return 0;     // (per-tap lane tables, 32-bit slice offsets)
    if (!(d->in_slope >= 0.f && d->in_slope <= 1.f)) return 0;
    if ((long)d->Hin * d->Win * d->Cin >= (1L << 31) || (long)d->Hout * d->Wout >= (1L << 31)) return 0;
    if (((size_t)d->x | (size_t)d->w | (size_t)d->out | (size_t)d->res | (size_t)d->res2 | (size_t)d->mask_src |
         (size_t)d->bias) & 15)
        return 0;
    if (bn >= 2 * d->Cout && bn > 64) return 0;                 // more than half of the tile would be padding
    // stages per barrier: 1, 2, or all taps of a chunk (the halo request then always precedes the super-stage that reads it)
    if (!(spb == 1 || spb == 2 || spb == d->ntaps)) return 0;
    size_t unused;
    int rc = cv_geometry(d, &pl->G, 2, 72, bn, &unused, bm);
    if (rc) return rc;
    const long npix = (long)pl->G.IH * pl->G.IW;
    if (npix > 64L * xv) return 0;
    if (xv > 3 && npix <= 64L * 3 && bm <= 128) return 0;       // (the three-instruction forms take it)
    const size_t xbytes = (((size_t)npix * 128) + 1023) & ~(size_t)1023;
    size_t work = 2 * xbytes + (size_t)2 * spb * bn * 128;
    const size_t xch = kg >= 2 ? (size_t)CV7_WAVES * 2 * 16 * 64 * 4 : 0;      // exchange area of the contraction groups
    if (work < xch) work = xch;
    const size_t lds = 1024 + work;
    if (lds > 160 * 1024) return 0;
    pl->applies = 1;
    pl->cfg = variant - 56;
    pl->lds = lds;
    pl->tilesM = pl->G.tilesX * pl->G.tilesY * d->B;
    pl->tilesN = (d->Cout + bn - 1) / bn;
    pl->blocks = ((pl->tilesM + 7) / 8) * 8 * pl->tilesN;
    return 0;
}

static int cv7_dispatch(const Cv7Plan& pl, unsigned blocks, size_t lds, msmc_stream stream, const msmc_conv_desc* d,
                        const Cv7GroupArgs* group) {
    int rc;
    const Cv7Run R = {pl.tilesM, pl.tilesN};
#define CV7_INST(WM_, WN_, KG_, SPB_, XV_)                                                                            \
    do {                                                                                                           \
        if (group) {                                                                                               \
            rc = msmc_allow_lds((const void*)conv_gather7_group_kernel<WM_, WN_, KG_, SPB_, XV_>, (int)lds);      \
            if (rc) return rc;                                                                                     \
            MSMC_LAUNCH((conv_gather7_group_kernel<WM_, WN_, KG_, SPB_, XV_>), dim3(blocks), dim3(512), lds,      \
                        (msmc_stream_t)stream, *group);                                                            \
        } else {                                                                                                   \
            rc = msmc_allow_lds((const void*)conv_gather7_kernel<WM_, WN_, KG_, SPB_, XV_>, (int)lds);            \
            if (rc) return rc;                                                                                     \
            MSMC_LAUNCH((conv_gather7_kernel<WM_, WN_, KG_, SPB_, XV_>), dim3(blocks), dim3(512), lds,            \
                        (msmc_stream_t)stream, *d, pl.G, R);                                                       \
        }                                                                                                          \
    } while (0)
    switch (pl.cfg) {
        case 0: CV7_INST(2, 2, 2, 1, 3); break;
        case 3: CV7_INST(1, 2, 4, 2, 3); break;
        case 4: CV7_INST(4, 2, 1, 2, 5); break;
        case 5: CV7_INST(2, 1, 4, 2, 3); break;
        case 7: CV7_INST(2, 2, 2, 2, 3); break;
        default: return MSMC_E_SHAPE;
    }
#undef CV7_INST
    static thread_local char name[96];
    int wm, wn, kg, spb, xv;
    cv7_cfg(pl.cfg, &wm, &wn, &kg, &spb, &xv);
    // (the symbol as rocprofv3 prints it: bench.py joins its launch log with the PMC passes by name)
    snprintf(name, sizeof(name), "%s<%d, %d, %d, %d, %d>", group ? "conv_gather7_group_kernel" : "conv_gather7_kernel", wm, wn, kg, spb, xv);
    msmc_conv_last = msmc_prof_name(name);
    return msmc_check_launch();
}

// one descriptor on the seventh generation: 1 = launched, 0 = does not apply, < 0 error
static int cv7_launch(const msmc_conv_desc* d, msmc_stream stream) {
    Cv7Plan pl;
    int rc = cv7_plan(d, d->variant, &pl);
    if (rc) return rc;
    if (!pl.applies) return 0;
    rc = cv7_dispatch(pl, (unsigned)pl.blocks, pl.lds, stream, d, nullptr);
    return cv_launched(rc);
}

// members of a grouped call (cv_family_group_launch): one grid per configuration
struct Cv7Family {
    typedef Cv7Plan Plan;
    typedef Cv7GroupArgs Args;
    static constexpr int min_members = 1;
    static constexpr bool lone_single = true;
    static bool mine(const msmc_conv_desc* d) { return cv7_is_variant(d->variant); }
    static int plan(const msmc_conv_desc* d, Plan* pl, int) { return cv7_plan(d, d->variant, pl); }
    static bool same(const Plan& p, const Plan& q) { return p.cfg == q.cfg; }
    static int blocks(const Plan& p) { return p.blocks; }
    static int* head(Args& ga, int m) { ga.a.n = m; return ga.a.first; }
    static void fill(Args& ga, int k, const msmc_conv_desc& d, const Plan& p) {
        ga.a.nx[k] = p.blocks;
        ga.a.d[k] = d;
        ga.a.G[k] = p.G;
        ga.R[k] = Cv7Run{p.tilesM, p.tilesN};
    }
    static int dispatch(const Plan& p, int blocks, size_t lds, msmc_stream stream, const msmc_conv_desc* d, const Args* group) {
        return cv7_dispatch(p, (unsigned)blocks, lds, stream, d, group);
    }
};
