// wgrad7.inc -- bf16 weight gradient on 128 x 128 channel tiles (descriptor variant 9; included by conv_wgrad.hip after wgrad6.inc).
//
// Reference layers: the k = 3 feed-forward convolutions of the predictor's FFT blocks at B = 64 (600 <-> 1536 channels over
// 25 600 frames: msmctts/networks/acoustic_models/transformer.py:330-352, examples/csmsc/configs/msmc_vq_gan_am.yaml) -- any
// unit-stride layer with >= 128 channels on both sides and a pixel count that fills the chip at this tile size.
//
// Why: the fourth generation's workgroup owns 64 x 64 channels, so every 64-channel x tile is fetched once per 64 output
// channels and every g tile once per 64 input channels -- at 600 <-> 1536 the L2 -> LDS stream is 17 x the algorithmic bytes
// (1.9 GB per launch at 9 TB/s) and, measured with the two phases switched off in turn (profiles/r05_wgrad4_am_splits.txt),
// the stream (267 us) and the MFMA + fragment-read phase (180 us) ADD UP to the launch (380 us).  Here a workgroup of EIGHT
// waves owns 128 x 128 channels: half the staged bytes per flop, and a wave owns 64 output x 32 input channels x TPW taps --
// two A fragments and TPW B fragments for 2 TPW MFMAs per 16-pixel step (wgrad4: 1 + TPW fragments for TPW MFMAs).
// Measured at 600 -> 1536, k = 3, 25 600 frames (profiles/r05_wgrad7_am_splits.txt): 250 us against the fourth generation's 383
// (566 TFLOP/s); the request stream alone 142 us (0.94 GB out of L2 at 10 TB/s: its roof), the MFMA + fragment phase alone 160 us,
// still adding up.  Tried on top and dropped: the two waves of a SIMD requesting at opposite ends of a tile (253 against 246 us)
// and a second fragment set requested one step ahead (254 us; the MFMA phase alone 171); per-instruction request tables worked out
// once per workgroup instead of the region tests, row products and the division per tile below (~100 instructions per request,
// 9 scalar + 5 vector instructions per MFMA over the launch: profiles/r05_wgrad7_sq_counters.txt): 251 us -- the request stream is
// bound by L2 (0.94 GB in 94 us), not by its instruction count.
//
// Everything else is wgrad4.inc's: scope (bf16, unit strides, zero padding, taps along one axis, channel counts multiples
// of 8), the flattened pixel axis, the ring of NS pixel-tile stages filled by LDS-DMA with the source-side swizzle (rows
// with bit 1 set hold their 64-byte halves swapped), ONE LDS-only barrier per tile, split partial results summed in split
// order by conv_wgrad_reduce_kernel.  LDS image of a stage: the two 64-channel halves of the output-gradient tile (TM rows
// each), then the two halves of the x tile (XR rows each), 128 bytes per row.
// The 16-pixel steps of one tile as ONE loop body (not straight-line code per step count, and no bias / no-bias copies of it):
// with several copies of the MFMA region hipcc gave the accumulators a second set of "home" registers that the copies move
// results to and from -- 72 registers per tap instead of 39, a spilling kernel at three taps.  ONE fragment set: the reads of step
// ks + 1 are issued right after the MFMAs of step ks (into the registers those MFMAs have read) and land while they drain.
template <int TPW>
MSMC_DEV void wg7_tile(const int nks, const unsigned short* gt, const unsigned short* xt, const int (&aoff)[2],
                       const int (&boff)[TPW], f32x16 (&acc)[TPW][2], float (&bsum)[2], const bool bias_wave) {
    const unsigned short* ap0 = gt + aoff[0];
    const unsigned short* ap1 = gt + aoff[1];
    const unsigned short* bp[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j) bp[j] = xt + boff[j];
    Wg4Frag a0 = wg4_read<0>(ap0), a1 = wg4_read<0>(ap1), b[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j) b[j] = wg4_read<0>(bp[j]);
#pragma unroll 1
    for (int ks = 0; ks < nks; ++ks) {
        lds_wait<0>();
        const bf16x8 af0 = wg4_frag(a0), af1 = wg4_frag(a1);
        if (bias_wave) {
            const u16x8 ab0 = __builtin_bit_cast(u16x8, af0), ab1 = __builtin_bit_cast(u16x8, af1);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                bsum[0] = bsum[0] + bf16_bits_to_f32(ab0[q]);
                bsum[1] = bsum[1] + bf16_bits_to_f32(ab1[q]);
            }
        }
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
            const bf16x8 bf = wg4_frag(b[j]);
            acc[j][0] = mfma_bf16_32x32x16(af0, bf, acc[j][0]);
            acc[j][1] = mfma_bf16_32x32x16(af1, bf, acc[j][1]);
        }
        if (ks + 1 < nks) {                                     // next step: sixteen rows further down both images
            ap0 += 1024;
            ap1 += 1024;
            a0 = wg4_read<0>(ap0);
            a1 = wg4_read<0>(ap1);
#pragma unroll
            for (int j = 0; j < TPW; ++j) {
                bp[j] += 1024;
                b[j] = wg4_read<0>(bp[j]);
            }
        }
    }
}

template <int TPW>
__global__ __launch_bounds__(512) void conv_wgrad7_kernel(msmc_conv_desc d, const unsigned short* __restrict__ gptr,
                                                          float* __restrict__ dw, float* __restrict__ db, Wg4Params P) {
    MSMC_DYN_LDS(smem);
    unsigned short* ring = (unsigned short*)smem;
    const int block_x = blockIdx.x, block_y = blockIdx.y, block_z = blockIdx.z;
    const int TM = P.TM, XR = P.XR, NS = P.NS;
    const int stage = 2 * (TM + XR) * 64;                        // elements per ring stage
    const int tid = threadIdx.x, w = wave_uniform(tid >> 6), lane = tid & 63, L = lane & 15, half = (lane >> 4) & 1;
    const int g = lane >> 5;
    const int co0 = block_y * 128;
    const int ciTile = block_z / P.ntg, tg = block_z - ciTile * P.ntg;
    const int ci0 = ciTile * 128;
    // this wave: output-channel half wco (both 32-channel blocks of it), input-channel half xh, 32-channel block ib of it
    const int wco = w & 1, wci = w >> 1, xh = wci >> 1, ib = wci & 1;
    const int tap0 = tg * P.TG;
    int ntl = d.ntaps - tap0;
    if (ntl > P.TG) ntl = P.TG;
    const int frow = 8 * g + (L >> 2);                           // row this lane addresses inside a 16-row step
    int boff[TPW], utap[TPW], aoff[2];
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        utap[j] = j < ntl ? tap0 + j : -1;                        // (units past the tap range compute on shift 0, never stored)
        const int row = frow + (j < ntl ? P.toff[tap0 + j] : 0);
        boff[j] = row * 64 + ((32 * ib + 16 * half + 4 * (L & 3)) ^ (((row >> 1) & 1) << 5));
    }
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) aoff[cb] = frow * 64 + ((32 * cb + 16 * half + 4 * (L & 3)) ^ (((frow >> 1) & 1) << 5));
    f32x16 acc[TPW][2];
#pragma unroll
    for (int j = 0; j < TPW; ++j)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][cb][r] = 0.f;

    const bool partial = P.ws != nullptr;
    if (partial) {
        dw = P.ws + (size_t)block_x * P.ws_stride;
        if (db) db = dw + (size_t)d.ntaps * d.Cout * d.Cin;
    }
    const bool bias_wave = (db != nullptr) && (block_z == 0) && (wci == 0);
    float bsum[2] = {0.f, 0.f};
    const int nks = TM >> 4;
    const int t0 = block_x * P.tilesPerWg;
    int t1 = t0 + P.tilesPerWg;
    if (t1 > P.totalTiles) t1 = P.totalTiles;

    // ---- LDS-DMA of one tile: instruction q = eight 128-byte rows of the stage image; wave w issues q = w, w + 8, ...
    const int drow = lane >> 3;                                  // row of this lane inside an instruction
    const int dchunk = ((lane & 7) ^ (((drow >> 1) & 1) << 2)) * 8;   // SOURCE channel offset (halves swapped on rows 2, 3, 6, 7)
    const unsigned short* xbase = (const unsigned short*)d.x + ci0 + dchunk;
    const unsigned short* gbase = gptr + co0 + dchunk;
    const bool gpiece[2] = {co0 + dchunk < d.Cout, co0 + 64 + dchunk < d.Cout};
    const bool xpiece[2] = {ci0 + dchunk < d.Cin, ci0 + 64 + dchunk < d.Cin};
    auto issue = [&](int tile, unsigned short* st) {
        const int b = tile / P.tilesPerImg;
        const int p0 = (tile - b * P.tilesPerImg) * TM;
        const unsigned short* gtile = gbase + ((size_t)b * P.Pout + p0) * d.Cout;
        const unsigned short* xtile = xbase + ((ptrdiff_t)b * P.Pin + p0 + P.offmin) * d.Cin;
        for (int k = 0; k < P.npw; ++k) {
            const int q = w + 8 * k;
            int r0 = 8 * q;
            const void* src = (const void*)msmc_wg4_zero_chunk;
            if (r0 < 2 * TM) {
                const int hh = r0 >= TM;
                r0 -= hh * TM;
                if (gpiece[hh] && p0 + r0 + drow < P.Pout) src = gtile + (size_t)(r0 + drow) * d.Cout + 64 * hh;
            } else {
                r0 -= 2 * TM;
                const int hh = r0 >= XR;
                r0 -= hh * XR;
                const int ip = p0 + P.offmin + r0 + drow;
                if (xpiece[hh] && ip >= 0 && ip < P.Pin) src = xtile + (ptrdiff_t)(r0 + drow) * d.Cin + 64 * hh;
            }
            lds_dma16(src, st + (size_t)q * 512);
        }
    };

    const bool dma_on = !(P.ablate & 2), mfma_on = !(P.ablate & 1);
    for (int s = 0; s < NS - 1; ++s)
        if (t0 + s < t1 && dma_on) issue(t0 + s, ring + (size_t)s * stage);
    int cur_s = 0;
    for (int tile = t0; tile < t1; ++tile) {
        const int rem = t1 - 1 - tile;
        wg4_dma_wait((rem < NS - 2 ? rem : NS - 2) * P.npw);     // this tile has landed; younger ones may still fly
        block_sync_lds();                                        // ... for every wave, and tile-1 is consumed
        int nxt_s = cur_s + NS - 1;
        if (nxt_s >= NS) nxt_s -= NS;
        if (tile + NS - 1 < t1 && dma_on) issue(tile + NS - 1, ring + (size_t)nxt_s * stage);
        unsigned short* gt = ring + (size_t)cur_s * stage;
        unsigned short* xt = gt + 2 * TM * 64;
        if (++cur_s == NS) cur_s = 0;
        if (d.in_slope != 1.f) {                                 // input activation in place (zero rows stay zero)
            for (int e = tid; e < 2 * XR * 8; e += 512) {
                u32x4 v = *(const u32x4*)(xt + (size_t)e * 8);
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = bf16x2_leaky(v[q], d.in_slope);
                *(u32x4*)(xt + (size_t)e * 8) = v;
            }
            block_sync_lds();
        }
        const unsigned short* ga = gt + (size_t)wco * TM * 64;
        const unsigned short* xa = xt + (size_t)xh * XR * 64;
        wg7_tile<TPW>(mfma_on ? nks : 0, ga, xa, aoff, boff, acc, bsum, bias_wave);   // (diagnostics: no steps)
    }

    if (bias_wave) {
        // lane (i, g) summed output channel 64 wco + 32 cb + i over the pixels 8g .. 8g + 7 of every 16-pixel step
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            const float bs = bsum[cb] + wave_xor(bsum[cb], 32);
            const int co = co0 + 64 * wco + 32 * cb + (lane & 31);
            if (g == 0 && co < d.Cout) {
                float* q = db + co;
                *q = partial ? bs : *q + bs;
            }
        }
    }
    // D fragment: row (co) = 64 wco + 32 cb + (r & 3) + 8 (r >> 2) + 4 g, col (ci) = 64 xh + 32 ib + (lane & 31)
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        if (utap[j] < 0) continue;
        const int ci = ci0 + 64 * xh + 32 * ib + (lane & 31);
        if (ci >= d.Cin) continue;
        float* dst = dw + (size_t)d.tap_w[utap[j]] * d.Cout * d.Cin;
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + 64 * wco + 32 * cb + (r & 3) + 8 * (r >> 2) + 4 * g;
                if (co >= d.Cout) continue;
                float* q = dst + (size_t)co * d.Cin + ci;
                *q = partial ? acc[j][cb][r] : *q + acc[j][cb][r];
            }
    }
}

// scope and pixel geometry as wg4_plan; 128-channel tiles, at most four taps per workgroup, one workgroup per CU
static int wg7_plan(const msmc_conv_desc* d, const void* g, Wg4Plan* pl) {
    if (d->dtype != 1 || d->pad_mode != 0 || d->mask_slope != 1.f) return MSMC_E_SHAPE;
    if (!(d->in_slope >= 0.f && d->in_slope <= 1.f)) return MSMC_E_SHAPE;
    if ((d->Cin & 7) || (d->Cout & 7) || d->Cin < 128 || d->Cout < 128) return MSMC_E_SHAPE;
    if (d->isy != 1 || d->isx != 1 || d->osy != 1 || d->osx != 1 || d->oy0 || d->ox0 || d->QH != d->Hout ||
        d->QW != d->Wout)
        return MSMC_E_SHAPE;
    if ((((size_t)d->x) | ((size_t)g)) & 15) return MSMC_E_SHAPE;
    bool along_w = d->Hin == 1 && d->Hout == 1 && d->iy0 == 0, along_h = d->Win == d->Wout && d->ix0 == 0;
    for (int t = 0; t < d->ntaps; ++t) {
        if (d->tap_dy[t] != 0) along_w = false;
        if (d->tap_dx[t] != 0) along_h = false;
    }
    if (!along_w && !along_h) return MSMC_E_SHAPE;
    Wg4Params& P = pl->P;
    P.ws = nullptr;
    P.ablate = msmc_wg4_ablate;
    P.Pin = d->Hin * d->Win;
    P.Pout = d->Hout * d->Wout;
    int off[MSMC_CONV_MAX_TAPS], offmin = 0, offmax = 0;
    for (int t = 0; t < d->ntaps; ++t) {
        off[t] = (d->iy0 + d->tap_dy[t]) * d->Win + d->ix0 + d->tap_dx[t];
        if (t == 0 || off[t] < offmin) offmin = off[t];
        if (t == 0 || off[t] > offmax) offmax = off[t];
    }
    const int span = offmax - offmin;
    if (span > 1024) return MSMC_E_SHAPE;
    P.offmin = offmin;
    for (int t = 0; t < MSMC_CONV_MAX_TAPS; ++t) P.toff[t] = t < d->ntaps ? off[t] - offmin : 0;
    int best = 8;
    long bestPad = -1;
    for (int nk = 8; nk >= 4; --nk) {                            // the step count that wastes the least of an image's last tile
        const long tiles = (P.Pout + 16 * nk - 1) / (16 * nk), pad = tiles * nk;
        if (bestPad < 0 || pad < bestPad) { bestPad = pad; best = nk; }
    }
    P.TM = 16 * best;
    P.XR = ((2 * P.TM + span + 31) & ~31) - P.TM;               // 2 (TM + XR) / 8 instructions: a multiple of the 8 waves
    P.npw = (P.TM + P.XR) / 32;
    const size_t stage_bytes = (size_t)2 * (P.TM + P.XR) * 128;
    P.NS = 3;
    while (P.NS > 2 && P.NS * stage_bytes > 160 * 1024) --P.NS;
    if (P.NS * stage_bytes > 160 * 1024 || (P.NS - 2) * P.npw > 32) return MSMC_E_SHAPE;
    pl->lds = P.NS * stage_bytes;
    int tgmax = msmc_wgrad_tpw_cap < 4 ? msmc_wgrad_tpw_cap : 4;  // taps per workgroup: 2 accumulators per tap and wave
    if (tgmax < 1) tgmax = 1;
    P.ntg = (d->ntaps + tgmax - 1) / tgmax;
    P.TG = (d->ntaps + P.ntg - 1) / P.ntg;
    pl->tpw = P.TG;
    P.tilesPerImg = (P.Pout + P.TM - 1) / P.TM;
    P.totalTiles = P.tilesPerImg * d->B;
    const int coT = (d->Cout + 127) / 128, ciT = (d->Cin + 127) / 128;
    const int cols = coT * ciT * P.ntg;
    int nsplit = (2 * MSMC_NUM_CU) / cols;                       // one workgroup per CU: two rounds of them
    if (nsplit < 1) nsplit = 1;
    if (d->split_shift > 0) nsplit <<= d->split_shift;
    else if (d->split_shift < 0) nsplit >>= -d->split_shift;
    const long n_dw = (long)d->ntaps * d->Cout * d->Cin;
    const long stride = ((n_dw + d->Cout + 3) / 4) * 4;
    const long fit = WG3_WS_CAP_FLOATS / stride;
    if (nsplit > fit) nsplit = (int)(fit > 1 ? fit : 1);
    if (msmc_wgrad_split_override > 0) nsplit = msmc_wgrad_split_override;
    if (nsplit > P.totalTiles) nsplit = P.totalTiles;
    if (nsplit < 1) nsplit = 1;
    P.tilesPerWg = (P.totalTiles + nsplit - 1) / nsplit;
    nsplit = (P.totalTiles + P.tilesPerWg - 1) / P.tilesPerWg;
    P.direct = nsplit == 1;
    P.ws_stride = stride;
    pl->ws_floats = nsplit > 1 ? (size_t)(nsplit + wg3_reduce_plan(n_dw + d->Cout, nsplit).groups) * stride : 0;
    pl->gx = (unsigned)nsplit;
    pl->gy = (unsigned)coT;
    pl->gz = (unsigned)(ciT * P.ntg);
    return 0;
}

static int wg7_launch(const msmc_conv_desc* d, const void* g, float* dw, float* db, msmc_stream stream, float* ws,
                      size_t ws_floats) {
    Wg4Plan pl;
    int rc = wg7_plan(d, g, &pl);
    if (rc) return rc;
    rc = wg3_take_ws(pl.ws_floats, ws, ws_floats, &pl.P.ws);
    if (rc) return rc;
    const dim3 grid(pl.gx, pl.gy, pl.gz);
    const unsigned short* gp = (const unsigned short*)g;
#define WG7_GO(TP)                                                                                           \
    do {                                                                                                     \
        rc = msmc_allow_lds((const void*)conv_wgrad7_kernel<TP>, (int)pl.lds);                               \
        if (rc) return rc;                                                                                   \
        MSMC_LAUNCH((conv_wgrad7_kernel<TP>), grid, dim3(512), pl.lds, (msmc_stream_t)stream, *d, gp, dw, db, pl.P); \
    } while (0)
    if (pl.tpw == 1) WG7_GO(1);
    else if (pl.tpw == 2) WG7_GO(2);
    else if (pl.tpw == 3) WG7_GO(3);
    else WG7_GO(4);
#undef WG7_GO
    msmc_conv_last = msmc_prof_name(msmc_kname("conv_wgrad7_kernel", nullptr, pl.tpw, -1));
    rc = msmc_check_launch();
    if (rc || !pl.P.ws) return rc;
    return wg3_reduce_single(d, ws, pl.P.ws_stride, (int)pl.gx, dw, db, stream);
}
