// gather5.inc -- fifth-generation bf16 forward / data-gradient implicit GEMM (variants 40..47; included by conv.hip).
//
// Same descriptor semantics as the third generation (lattice + tap table + padding rule + input activation + epilogue;
// reference layers: the k = 3 feed-forward convolutions of the FFT blocks, acoustic_models/transformer.py:330-352, the
// HifiGAN ResBlock / MRF convolutions, msmctts/networks/hifigan/common.py:21-57, the k x 1 period-discriminator and 3 x 3
// resolution-discriminator stacks, msmctts/networks/hifigan/discriminator.py:15-154), the machine mapping of the 1-tap GEMM (gemm1.inc) instead of
// gather3's: the third generation runs FOUR waves per workgroup on a 128 x 64 tile with all taps' weight slices of a
// chunk staged at once (80+ KB of LDS: one workgroup, i.e. one wave per SIMD, per CU) and one barrier + one memory
// round trip per chunk, which prices these 10-60 GFLOP layers at 6-12 % of the matrix-core peak.  Here:
//   * SIXTEEN waves per workgroup (four per SIMD hide each other's LDS / epilogue latency), tile = (32 PB MW) lattice
//     points x (32 CB 16/MW) output channels, PB x CB accumulators of v_mfma_f32_32x32x16_bf16 per wave;
//   * the contraction runs over STAGES s = (64-channel chunk c, tap t): a stage needs only the tap's weight slice of the
//     chunk (BN rows x 128 B = 16-32 KB) -- the halo tile of the chunk is shared by its taps (two buffers) -- so a ring
//     of S = 3..4 weight stages fits beside it and S-1 stages are in flight under the MFMAs of the current one, ONE
//     LDS-only barrier per stage, counted waits (s_waitcnt vmcnt(N): every wave issues the same number of LDS-DMA
//     instructions per stage -- pieces past the tile or past the last stage copy a zero chunk -- so N is a constant);
//   * both operands travel by LDS-DMA (no staging registers), rows of 128 B with the 16-byte pieces XOR-ed by
//     (row >> 1) & 7 at the SOURCE: conflict-free ds_read_b128 fragments for unit-stride lattices;
//   * operand roles swapped (A = weight rows, B = halo pixels) and one v_permlane32_swap per accumulator register pair:
//     a lane ends up with two runs of EIGHT consecutive channels of one lattice point -- bias / mask / residuals /
//     leaky-ReLU / bf16 pack in registers, 16-byte stores, no LDS round trip in the epilogue;
//   * workgroups of one pixel tile are numbered onto one XCD (the halo tile is re-read from its L2).
// Requirements (cv5_plan refuses the rest, the tuner then drops the candidate): bf16, Cin % 64 == 0, Cout % 8 == 0, at
// least two taps (one: gemm1.inc), halo tile of at most 384 pixels, 0 <= in_slope <= 1.
#include <type_traits>
#define CV5_XV 3                                           // LDS-DMA instructions per wave and halo-tile chunk

struct Cv5Plan {
    int applies;
    int cfg;                                               // 0..4: (PB, CB, MW) below
    int S;                                                 // weight-ring stages
    CvGeom G;
    size_t lds;
    int tilesM, tilesN, blocks;
};
struct Cv5Run {
    int S, tilesM, tilesN;
};

// padding pixels and pieces past the halo tile read zeros from here; the chunk offset (< 2 * Cin bytes) is added to every
// source alike, so the page covers the widest input row cv5_plan admits
#define CV5_MAX_CIN 2048
__device__ const u32x4 msmc_cv5_zero_page[CV5_MAX_CIN * 2 / 16 + 8] = {};

// the two lanes (i, 0) and (i, 1) of a 32x32 accumulator column hold the channel runs {8q + 4g .. +3}: after the swap
// of the register pairs (q even, q odd) lane g holds the eight consecutive channels 16 (q / 2) + 8 g + (0 .. 7)
MSMC_DEV void cv5_swap_runs(f32x16& acc) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            unsigned int a = __float_as_uint(acc[8 * h + j]), b = __float_as_uint(acc[8 * h + 4 + j]);
            wave_swap32(a, b);
            acc[8 * h + j] = __uint_as_float(a);
            acc[8 * h + 4 + j] = __uint_as_float(b);
        }
}

// One stage (64-channel chunk, tap) of the contraction in ring slot SLOT.  VALU discipline: a 32x32x16 MFMA leaves the
// vector ALU port free for about seven instructions, and with four waves per SIMD every per-stage instruction of a wave is
// paid four times -- so per-lane addresses are loop invariants (weight fragments: register + immediate slot offset; LDS-DMA
// sources: per-lane 64-bit bases + a scalar stage offset), per-tap quantities come from lane tables by v_readlane, and
// the only per-stage vector arithmetic is the halo-fragment addresses (the tap shift moves rows AND their swizzle key).
struct Cv5Loop {
    int c, t, s;                       // chunk, tap, flattened stage of the stage being computed
    int ic, it;                        // (chunk, tap) of the next weight stage to request
};

// KS = 2: the sixteen waves are TWO groups of eight that each run half of the channel chunks of the SAME (smaller) tile
// through a ring and halo buffers of their own, on the same stage cadence (one barrier serves both); at the end the second
// group's accumulators go through LDS and the first group adds them (fixed order) and runs the epilogue.  For the layers
// with few lattice points and deep contractions (1024 -> 256 FFN convolution, C256 x L240 ResBlocks, 512 -> 512
// period-discriminator layers: 64-128 workgroups of 40-90 serial stages otherwise): four times the parallelism per layer.
// XV = LDS-DMA instructions per wave and halo-tile chunk.  XV = 5 is the form for ONE-chunk layers with wide halos (Cin = 64,
// strides 2 / 3: the 64 -> 128 resolution-discriminator layer's halo is 561 pixels for 128 outputs): a single halo buffer
// (there is no next chunk to prefetch) of up to 640 pixels.
template <int PB, int CB, int MW, int S, int KS, int XV>
MSMC_DEV void cv5_body(const msmc_conv_desc& d, const CvGeom& G, const Cv5Run& R, const int id) {
    MSMC_DYN_LDS(smem);
    typedef unsigned short T;
    constexpr bool SINGLE = XV > CV5_XV;                        // one chunk, one halo buffer
    constexpr int GW = 16 / KS;                                 // waves of a contraction group
    constexpr int NWV = GW / MW, BM = 32 * PB * MW, BN = 32 * CB * NWV;
    // a wave brings RPW weight rows per stage: whole LDS-DMA instructions of eight rows, or ONE instruction with half of its
    // lanes active (64-channel tiles: four rows) -- either way every wave issues the same number of instructions per stage
    constexpr int RPW = BN / GW, WP = RPW >= 8 ? RPW / 8 : 1, WLANES = RPW >= 8 ? 64 : RPW * 8;
    static_assert(BN % GW == 0 && (RPW % 8 == 0 || RPW == 4), "weight rows per wave and stage");
    constexpr int WST = BN * 128;
    const int npix = G.IH * G.IW, IW = G.IW;
    int* in_off = (int*)smem;                                   // [npix] element offset of halo pixel, -1 = zero
    int* out_off = in_off + npix;                               // [BM]   pixel index of lattice point, -1 = none
    char* region = smem + (((size_t)(npix + BM) * sizeof(int) + 1023) & ~(size_t)1023);
    char* dump = region;                                        // 1 KB: destination of the pieces past the halo tile
    const int xbytes = (npix * 128 + 1023) & ~1023;
    const int tid = threadIdx.x, w = wave_uniform(tid >> 6), lane = tid & 63, li = lane & 31, g = lane >> 5;
    const int kg = w / GW, wl = w - kg * GW;                    // contraction group, wave within it
    constexpr int NXB = SINGLE ? 1 : 2;                         // halo buffers
    char* xbuf0 = region + 1024 + kg * (NXB * xbytes + S * WST);        // this group's halo buffers ...
    char* wring = xbuf0 + NXB * xbytes;                         // ... and ring: S stages of [BN rows][128 B]
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
    const int wm_ = wl % MW, wn_ = wl / MW;
    const int Cin = d.Cin, Cout = d.Cout;
    const int nchunks = (Cin >> 6) / KS, ntaps = d.ntaps;      // (this group's chunks: kg * nchunks + 0 .. nchunks-1)
    const int cbase = kg * nchunks * 128;                       // byte offset of the group's first chunk in a row
    const int nst = nchunks * ntaps;
    const int abl = d.split_shift;      // DIAGNOSTICS (0 in production; results are garbage otherwise): 2 no weight stream,
                                        // 4 no halo stream, 8 no epilogue, 32 no per-stage barrier (runtime branches on the
                                        // MFMA / fragment path cost accumulator copies: none there)

    const T* xb = (const T*)d.x + (size_t)b * d.Hin * d.Win * Cin;
    // per-tap lane tables (lane t): halo-tile row shift and byte offset of the tap's weight slice
    const int tl = lane < ntaps ? lane : 0;
    const int taprow_v = (d.tap_dy[tl] - G.dyMin) * IW + (d.tap_dx[tl] - G.dxMin);
    const unsigned int tapw_v = (unsigned int)d.tap_w[tl] * (unsigned int)Cout * (unsigned int)Cin * 2u;

    // ---- weight slice of a stage: WP instructions of eight rows each per wave; per-lane source of (chunk 0, slice 0)
    const char* wsrc[WP];
#pragma unroll
    for (int u = 0; u < WP; ++u) {
        const int n = wl * RPW + u * 8 + (lane >> 3);
        int co = co0 + n;
        if (co >= Cout) co = Cout - 1;                          // columns past Cout are never stored: any valid row
        wsrc[u] = (const char*)d.w + ((size_t)co * Cin + (((lane & 7) ^ ((n >> 1) & 7)) << 3)) * 2 + cbase;
    }
    Cv5Loop lp = {0, 0, 0, 0, 0};
    auto issue_w = [&](int slot) {                               // next stage (past the end: the last one again, never read)
        const size_t soff = (size_t)wave_read_lane(tapw_v, lp.it) + (size_t)lp.ic * 128;
        char* st = wring + slot * WST + wl * (RPW * 128);
#pragma unroll
        for (int u = 0; u < WP; ++u) {
            if (WLANES == 64 || lane < WLANES) lds_dma16(wsrc[u] + soff, st + u * 1024);
        }
        if (lp.ic * ntaps + lp.it + 1 < nst) {
            if (++lp.it == ntaps) { lp.it = 0; ++lp.ic; }
        }
    };
    if (!(abl & 2)) {
#pragma unroll
        for (int s = 0; s < S - 1; ++s) issue_w(s);              // in flight while the offset tables are built
    }

    for (int pi = tid; pi < npix; pi += 1024) {
        const int ry = pi / IW, rx = pi - ry * IW;
        int iy = iyBase + ry, ix = ixBase + rx;
        bool inside = true;
        if (d.pad_mode == 1) {
            iy = reflect_index(iy, d.Hin);
            ix = reflect_index(ix, d.Win);
        } else {
            inside = (iy >= 0) && (iy < d.Hin) && (ix >= 0) && (ix < d.Win);
        }
        in_off[pi] = inside ? (iy * d.Win + ix) * Cin : -1;
    }
    for (int m = tid; m < BM; m += 1024) {
        const int mty = m / G.TW, mtx = m - mty * G.TW;
        const int qy = qy0 + mty, qx = qx0 + mtx;
        const bool valid = mty < G.TH && qy < d.QH && qx < d.QW;
        out_off[m] = valid ? (d.oy0 + qy * d.osy) * d.Wout + (d.ox0 + qx * d.osx) : -1;
    }
    block_sync_lds();                                           // offset tables ready (LDS-only barrier: the first stages stay in flight)

    // halo tile by LDS-DMA: instruction q = wl + GW u covers eight pixels of one chunk; this lane's piece of it is the
    // same for every chunk: source-swizzled address in x, or the zero page for padding pixels / pieces past the tile
    const int nxq = (npix + 7) >> 3;
    const char* xsrc[XV];
#pragma unroll
    for (int u = 0; u < XV; ++u) {
        const int pi = (wl + GW * u) * 8 + (lane >> 3);
        xsrc[u] = (const char*)msmc_cv5_zero_page;
        if (pi < npix) {
            const int off = in_off[pi];
            if (off >= 0) xsrc[u] = (const char*)(xb + off + ((((lane & 7) ^ ((pi >> 1) & 7))) << 3)) + cbase;
        }
    }
    auto issue_x = [&](int c, int buf) {                        // (chunk past the end: the last one again, never read)
        const int cc = c < nchunks ? c : nchunks - 1;
        char* xbuf = xbuf0 + buf * xbytes;
#pragma unroll
        for (int u = 0; u < XV; ++u) {
            const int q = wl + GW * u;
            lds_dma16(xsrc[u] + cc * 128, q < nxq ? xbuf + q * 1024 : dump);
        }
    };
    if (!(abl & 4)) issue_x(0, 0);

    int arow[PB];
#pragma unroll
    for (int pb = 0; pb < PB; ++pb) {
        const int m = 32 * PB * wm_ + 32 * pb + li;
        const int mty = m / G.TW, mtx = m - mty * G.TW;
        arow[pb] = (mty < G.TH) ? (mty * d.isy) * IW + mtx * d.isx : 0;      // halo pixel of the lattice point at tap shift 0
    }
    // weight-fragment addresses inside slot 0 (the slot offset is an immediate of the read)
    const char* wfa[CB][4];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
        const int n = 32 * CB * wn_ + 32 * cb + li;
#pragma unroll
        for (int L = 0; L < 4; ++L) wfa[cb][L] = wring + n * 128 + (((2 * L + g) ^ ((n >> 1) & 7)) << 4);
    }
    f32x16 acc[CB][PB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int pb = 0; pb < PB; ++pb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[cb][pb][r] = 0.f;
    const float slope = d.in_slope;

    // waits: at the top of stage s the younger requests of this wave are the weight stages s+1 .. s+S-2 and, for taps
    // 1 .. S-2 of a chunk, the next chunk's halo tile (requested at tap 0, just before weight stage s+S-1)
    constexpr int WAIT_PLAIN = (S - 2) * WP, WAIT_HALO = SINGLE ? WAIT_PLAIN : WAIT_PLAIN + XV;
    auto stage = [&](auto slot_c) {
        constexpr int SLOT = decltype(slot_c)::value;
        if (lp.s == 0) lds_dma_wait();
        else if (lp.t >= 1 && lp.t < S - 1) lds_dma_wait_n<WAIT_HALO>();
        else lds_dma_wait_n<WAIT_PLAIN>();
        if (!(abl & 32)) block_sync_lds();                      // stage s landed for everyone; stage s-1's slot is free
        const char* xcur = xbuf0 + (lp.c & 1) * xbytes;
        if (lp.t == 0) {
            if (!(abl & 4) && !SINGLE) issue_x(lp.c + 1, (lp.c + 1) & 1);
            if (slope != 1.f) {                                 // input activation in place on the landed chunk, once
                for (int e = tid - kg * (64 * GW); e < npix * 8; e += 64 * GW) {
                    u32x4 v = *(const u32x4*)(xcur + e * 16);
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = bf16x2_leaky(v[q], slope);
                    *(u32x4*)(const_cast<char*>(xcur) + e * 16) = v;
                }
                block_sync_lds();
            }
        }
        if (!(abl & 2)) issue_w((SLOT + S - 1) % S);
        const int trow = wave_read_lane(taprow_v, lp.t);
        // fragments of k-slice L+1 in flight under the MFMAs of slice L (two register sets, source order kept)
        const char* xa[PB];
        int xkey[PB];
#pragma unroll
        for (int pb = 0; pb < PB; ++pb) {
            const int row = arow[pb] + trow;
            xa[pb] = xcur + (row << 7);
            xkey[pb] = (row >> 1) & 7;
        }
        auto read_slice = [&](auto L_c, u32x4 (&xf)[PB], u32x4 (&wf)[CB]) {
            constexpr int L = decltype(L_c)::value;
#pragma unroll
            for (int pb = 0; pb < PB; ++pb) xf[pb] = *(const u32x4*)(xa[pb] + (((2 * L + g) ^ xkey[pb]) << 4));
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) wf[cb] = *(const u32x4*)(wfa[cb][L] + SLOT * WST);
        };
        auto mma_slice = [&](const u32x4 (&xf)[PB], const u32x4 (&wf)[CB]) {
#pragma unroll
            for (int cb = 0; cb < CB; ++cb)
#pragma unroll
                for (int pb = 0; pb < PB; ++pb)
                    acc[cb][pb] = mfma_bf16_32x32x16(__builtin_bit_cast(bf16x8, wf[cb]), __builtin_bit_cast(bf16x8, xf[pb]), acc[cb][pb]);
            sched_fence();
        };
        u32x4 xf0[PB], wf0[CB], xf1[PB], wf1[CB];
        read_slice(std::integral_constant<int, 0>(), xf0, wf0);
        read_slice(std::integral_constant<int, 1>(), xf1, wf1);
        sched_fence();
        mma_slice(xf0, wf0);
        read_slice(std::integral_constant<int, 2>(), xf0, wf0);
        sched_fence();
        mma_slice(xf1, wf1);
        read_slice(std::integral_constant<int, 3>(), xf1, wf1);
        sched_fence();
        mma_slice(xf0, wf0);
        mma_slice(xf1, wf1);
#if defined(CV5_SALU_PAD) || defined(CV5_VALU_PAD)
        // SENSITIVITY BUILDS ONLY (tools/r04_pad_probe.sh; never defined by the Makefile): extra scalar / vector instructions per
        // stage, to read off what one more instruction of each kind costs the kernel
        {
#ifdef CV5_SALU_PAD
            int sp = __builtin_amdgcn_readfirstlane(lp.s);
#pragma unroll
            for (int q = 0; q < CV5_SALU_PAD; ++q) asm volatile("s_add_u32 %0, %0, 1" : "+s"(sp));
#endif
#ifdef CV5_VALU_PAD
            int vp = lane;
#pragma unroll
            for (int q = 0; q < CV5_VALU_PAD; ++q) asm volatile("v_add_u32 %0, %0, 1" : "+v"(vp));
#endif
        }
#endif
        ++lp.s;
        if (++lp.t == ntaps) { lp.t = 0; ++lp.c; }
    };
    while (lp.s < nst) {
        stage(std::integral_constant<int, 0>());
        if (lp.s < nst) stage(std::integral_constant<int, 1 % S>());
        if (S > 2 && lp.s < nst) stage(std::integral_constant<int, 2 % S>());
        if (S > 3 && lp.s < nst) stage(std::integral_constant<int, 3 % S>());
    }
    lds_dma_wait();                                             // (the repeated pieces of the stages past the end)
    if (KS == 2) {
        // second group -> LDS (lane-contiguous: conflict-free), first group adds: sum order (group 0) + (group 1)
        float* xch = (float*)(region + 1024);
        block_sync_lds();                                       // every wave is done with the stages
        if (kg == 1) {
#pragma unroll
            for (int cb = 0; cb < CB; ++cb)
#pragma unroll
                for (int pb = 0; pb < PB; ++pb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) xch[((wl * CB * PB + cb * PB + pb) * 16 + r) * 64 + lane] = acc[cb][pb][r];
        }
        block_sync_lds();
        if (kg == 1) return;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int pb = 0; pb < PB; ++pb)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[cb][pb][r] = acc[cb][pb][r] + xch[((wl * CB * PB + cb * PB + pb) * 16 + r) * 64 + lane];
    }

    // ---- epilogue in registers: lane (li, g) owns lattice point 32 PB wm + 32 pb + li and, after the swap, the channel
    // runs co0 + 32 CB wn + 32 cb + 16 h + 8 g + (0 .. 7), h = 0, 1
    const T* mask = (const T*)d.mask_src;
    const T* res = (const T*)d.res;
    const T* res2 = (const T*)d.res2;
    T* out = (T*)d.out;
    const size_t img = (size_t)b * d.Hout * d.Wout;
    const float mslope = d.mask_slope, odiv = d.out_div, oslope = d.out_slope;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int pb = 0; pb < PB; ++pb) cv5_swap_runs(acc[cb][pb]);
#pragma unroll
    for (int pb = 0; pb < PB; ++pb) {
        const int po = out_off[32 * PB * wm_ + 32 * pb + li];
        if (po < 0 || (abl & 8)) continue;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int n = co0 + 32 * CB * wn_ + 32 * cb + 16 * h + 8 * g;
                if (n >= Cout) continue;                        // (Cout % 8 == 0: a run is all in or all out)
                const size_t o = (img + po) * Cout + n;
                f32x4 b0 = {0.f, 0.f, 0.f, 0.f}, b1 = b0;
                if (d.bias) {
                    b0 = *(const f32x4*)(d.bias + n);
                    b1 = *(const f32x4*)(d.bias + n + 4);
                }
                u32x4 mk = {0u, 0u, 0u, 0u}, r1 = mk, r2 = mk;
                if (mask) mk = *(const u32x4*)(mask + o);
                if (res) r1 = *(const u32x4*)(res + o);
                if (res2) r2 = *(const u32x4*)(res2 + o);
                float ov[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) ov[j] = acc[cb][pb][8 * h + j] + (j < 4 ? b0[j & 3] : b1[j & 3]);
                {
                    const unsigned int mkw[4] = {mk[0], mk[1], mk[2], mk[3]}, r1w[4] = {r1[0], r1[1], r1[2], r1[3]},
                                       r2w[4] = {r2[0], r2[1], r2[2], r2[3]};
                    cv_ep<8>(ov, mkw, r1w, r2w, mask != nullptr, res != nullptr, res2 != nullptr, mslope, odiv, oslope);
                }
                const u32x4 pk = {pack_bf16x2(ov[0], ov[1]), pack_bf16x2(ov[2], ov[3]), pack_bf16x2(ov[4], ov[5]), pack_bf16x2(ov[6], ov[7])};
                *(u32x4*)(out + o) = pk;
            }
    }
}

template <int PB, int CB, int MW, int KS, int XV>
__global__ __launch_bounds__(1024) void conv_gather5_kernel(msmc_conv_desc d, CvGeom G, Cv5Run R) {
    if (KS == 1 && R.S == 4) cv5_body<PB, CB, MW, 4, KS, XV>(d, G, R, (int)blockIdx.x);
    else cv5_body<PB, CB, MW, 3, KS, XV>(d, G, R, (int)blockIdx.x);
}
struct Cv5GroupArgs {
    CvGroupArgs a;
    Cv5Run R[MSMC_GROUP_MAX];
};
template <int PB, int CB, int MW, int KS, int XV>
__global__ __launch_bounds__(1024) void conv_gather5_group_kernel(Cv5GroupArgs ga) {
    const int k = cv_group_member(ga.a.first, ga.a.n);
    if (KS == 1 && ga.R[k].S == 4) cv5_body<PB, CB, MW, 4, KS, XV>(ga.a.d[k], ga.a.G[k], ga.R[k], (int)blockIdx.x - ga.a.first[k]);
    else cv5_body<PB, CB, MW, 3, KS, XV>(ga.a.d[k], ga.a.G[k], ga.R[k], (int)blockIdx.x - ga.a.first[k]);
}

// variant 40 + cfg; (PB, CB, MW, KS) -> tile (lattice points x channels):
//   0: (1, 1, 4) 128 x 128    1: (2, 1, 4) 256 x 128    2: (1, 2, 4) 128 x 256    3: retired (round 6)      4: (1, 1, 2) 64 x 256
//   5: (1, 1, 2) in TWO contraction groups of eight waves: 64 x 128      6: (1, 1, 8) 256 x 64
//   7: (1, 1, 4) 128 x 128 for ONE-chunk layers (Cin = 64) with halo tiles of up to 640 pixels, single halo buffer
static bool cv5_is_variant(int variant) { return variant >= 40 && variant < 48; }
static void cv5_cfg(int cfg, int* pb, int* cb, int* mw, int* ks, int* xv = nullptr) {
    static const int T[8][5] = {{1, 1, 4, 1, 3}, {2, 1, 4, 1, 3}, {1, 2, 4, 1, 3}, {2, 1, 2, 1, 3}, {1, 1, 2, 1, 3}, {1, 1, 2, 2, 3},
                                {1, 1, 8, 1, 3}, {1, 1, 4, 1, 5}};
    *pb = T[cfg][0]; *cb = T[cfg][1]; *mw = T[cfg][2]; *ks = T[cfg][3];
    if (xv) *xv = T[cfg][4];
}

static int cv5_plan(const msmc_conv_desc* d, int variant, Cv5Plan* pl) {
    pl->applies = 0;
    if (d->dtype != 1 || !cv5_is_variant(variant)) return 0;
    if (variant == 43) return 0;       // (2, 1, 2) 128 x 256: retired in round 6 -- no decision of the tuned table over configurations 1-5
    int pb, cb, mw, ks, xv;
    cv5_cfg(variant - 40, &pb, &cb, &mw, &ks, &xv);
    const int bm = 32 * pb * mw, bn = 32 * cb * (16 / ks / mw);
    if (d->Cin % (64 * ks) != 0) return 0;                      // every contraction group runs the same number of chunks
    const bool single = xv > CV5_XV;
    if (single && d->Cin != 64) return 0;                       // (the single-buffer form: one chunk)
    if (d->Cin % 64 != 0 || d->Cin > CV5_MAX_CIN || d->Cout % 8 != 0 || d->ntaps < 2 || d->ntaps > MSMC_CONV_MAX_TAPS) return 0;
    if (d->ntaps > 64 || (double)d->ntaps * d->Cout * d->Cin * 2.0 >= 4294967296.0) return 0;     // (per-tap lane tables, 32-bit slice offsets)
    if (!(d->in_slope >= 0.f && d->in_slope <= 1.f)) return 0;
    if ((long)d->Hin * d->Win * d->Cin >= (1L << 31) || (long)d->Hout * d->Wout >= (1L << 31)) return 0;
    if (((size_t)d->x | (size_t)d->w | (size_t)d->out | (size_t)d->res | (size_t)d->res2 | (size_t)d->mask_src |
         (size_t)d->bias) & 15)
        return 0;
    if (bn >= 2 * d->Cout && bn > 64) return 0;                 // more than half of the tile would be padding
    size_t unused;
    int rc = cv_geometry(d, &pl->G, 2, 72, bn, &unused, bm);
    if (rc) return rc;
    const long npix = (long)pl->G.IH * pl->G.IW;
    if (npix > (128 / ks) * xv) return 0;
    if (single && npix <= 128 * CV5_XV) return 0;               // (the double-buffered forms take it)
    const size_t tables = (((size_t)(npix + bm) * sizeof(int)) + 1023) & ~(size_t)1023;
    const size_t xbytes = (((size_t)npix * 128) + 1023) & ~(size_t)1023;
    int S = (d->ntaps >= 3 && ks == 1) ? 4 : 3;
    const size_t nxb = single ? 1 : 2;
    size_t lds = tables + 1024 + (size_t)ks * (nxb * xbytes + (size_t)S * bn * 128);
    if (lds > 160 * 1024 && S == 4) {
        S = 3;
        lds = tables + 1024 + (size_t)ks * (nxb * xbytes + (size_t)S * bn * 128);
    }
    if (lds > 160 * 1024) return 0;
    if (ks == 2 && (size_t)ks * (nxb * xbytes + (size_t)S * bn * 128) < (size_t)8 * pb * cb * 16 * 64 * 4) return 0;   // (exchange area)
    pl->applies = 1;
    pl->cfg = variant - 40;
    pl->S = S;
    pl->lds = lds;
    pl->tilesM = pl->G.tilesX * pl->G.tilesY * d->B;
    pl->tilesN = (d->Cout + bn - 1) / bn;
    pl->blocks = ((pl->tilesM + 7) / 8) * 8 * pl->tilesN;
    return 0;
}

static int cv5_dispatch(const Cv5Plan& pl, unsigned blocks, size_t lds, msmc_stream stream, const msmc_conv_desc* d,
                        const Cv5GroupArgs* group) {
    int rc;
    const Cv5Run R = {pl.S, pl.tilesM, pl.tilesN};
#define CV5_INST(PB_, CB_, MW_, KS_, XV_)                                                                             \
    do {                                                                                                           \
        if (group) {                                                                                               \
            rc = msmc_allow_lds((const void*)conv_gather5_group_kernel<PB_, CB_, MW_, KS_, XV_>, (int)lds);             \
            if (rc) return rc;                                                                                     \
            MSMC_LAUNCH((conv_gather5_group_kernel<PB_, CB_, MW_, KS_, XV_>), dim3(blocks), dim3(1024), lds,            \
                        (msmc_stream_t)stream, *group);                                                            \
        } else {                                                                                                   \
            rc = msmc_allow_lds((const void*)conv_gather5_kernel<PB_, CB_, MW_, KS_, XV_>, (int)lds);                   \
            if (rc) return rc;                                                                                     \
            MSMC_LAUNCH((conv_gather5_kernel<PB_, CB_, MW_, KS_, XV_>), dim3(blocks), dim3(1024), lds,                  \
                        (msmc_stream_t)stream, *d, pl.G, R);                                                       \
        }                                                                                                          \
    } while (0)
    switch (pl.cfg) {
        case 0: CV5_INST(1, 1, 4, 1, 3); break;
        case 1: CV5_INST(2, 1, 4, 1, 3); break;
        case 2: CV5_INST(1, 2, 4, 1, 3); break;
        case 4: CV5_INST(1, 1, 2, 1, 3); break;
        case 5: CV5_INST(1, 1, 2, 2, 3); break;
        case 6: CV5_INST(1, 1, 8, 1, 3); break;
        default: CV5_INST(1, 1, 4, 1, 5); break;
    }
#undef CV5_INST
    static thread_local char name[96];
    int pb, cb, mw, ks, xv;
    cv5_cfg(pl.cfg, &pb, &cb, &mw, &ks, &xv);
    // (the symbol as rocprofv3 prints it: bench.py joins its launch log with the PMC passes by name)
    snprintf(name, sizeof(name), "%s<%d, %d, %d, %d, %d>", group ? "conv_gather5_group_kernel" : "conv_gather5_kernel", pb, cb, mw, ks, xv);
    msmc_conv_last = msmc_prof_name(name);
    return msmc_check_launch();
}

// one descriptor on the fifth generation: 1 = launched, 0 = does not apply, < 0 error
static int cv5_launch(const msmc_conv_desc* d, msmc_stream stream) {
    Cv5Plan pl;
    int rc = cv5_plan(d, d->variant, &pl);
    if (rc) return rc;
    if (!pl.applies) return 0;
    rc = cv5_dispatch(pl, (unsigned)pl.blocks, pl.lds, stream, d, nullptr);
    return cv_launched(rc);
}

// members of a grouped call (cv_family_group_launch): one grid per configuration
struct Cv5Family {
    typedef Cv5Plan Plan;
    typedef Cv5GroupArgs Args;
    static constexpr int min_members = 1;
    static constexpr bool lone_single = true;
    static bool mine(const msmc_conv_desc* d) { return cv5_is_variant(d->variant); }
    static int plan(const msmc_conv_desc* d, Plan* pl, int) { return cv5_plan(d, d->variant, pl); }
    static bool same(const Plan& p, const Plan& q) { return p.cfg == q.cfg; }
    static int blocks(const Plan& p) { return p.blocks; }
    static int* head(Args& ga, int m) { ga.a.n = m; return ga.a.first; }
    static void fill(Args& ga, int k, const msmc_conv_desc& d, const Plan& p) {
        ga.a.nx[k] = p.blocks;
        ga.a.d[k] = d;
        ga.a.G[k] = p.G;
        ga.R[k] = Cv5Run{p.S, p.tilesM, p.tilesN};
    }
    static int dispatch(const Plan& p, int blocks, size_t lds, msmc_stream stream, const msmc_conv_desc* d, const Args* group) {
        return cv5_dispatch(p, (unsigned)blocks, lds, stream, d, group);
    }
};
