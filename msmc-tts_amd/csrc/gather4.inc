// gather4.inc -- persistent bf16 forward / data-gradient kernel for the THIN long layers (included by conv.hip).
//
// The C <= 64 stages of the generator (ResBlocks over 6 000 / 12 000 samples) are priced by HBM, not by the matrix
// cores, and in generations 2 / 3 every workgroup of such a layer is one serial chain  load weights + halo -> barrier ->
// MFMA -> LDS tile -> barrier -> store  with one or two channel chunks -- nothing for the chunk pipeline to overlap.
// Here (descriptor variant 32; 33 = the same with the epilogue of a tile deferred into the next iteration, measured no
// faster -- profiles/r02_gather4d_first_measurement.txt -- and therefore not a tuner candidate):
//   * the weight rows of ALL taps, [tap][co][ci], are brought into LDS once per workgroup (LDS-DMA) and stay;
//   * the grid is persistent: a workgroup strides over the pixel tiles (128 output pixels each) of the whole batch, the
//     halo rows of the NEXT tile travel by LDS-DMA (global_load_lds_dwordx4, source-swizzled unpadded rows, zero chunk
//     outside the image) while the matrix cores work on the current one -- the pixel axis is flattened as in wgrad4.inc
//     (input pixel = output pixel + off[t], zero outside [0, Pin));
//   * operand roles are swapped against gather3: A = weight rows (output channels), B = halo rows (pixels), so the
//     accumulator holds [co][pixel] and a work-item owns four runs of four consecutive output channels of ONE pixel:
//     bias / mask / residuals / leaky-ReLU / bf16 pack run in registers and the stores are 8-byte vectors -- no fp32 LDS
//     tile, no epilogue barriers;
//   * the MFMA phase is gather3's: two fragment register sets, hand-counted LDS reads one step ahead, the tap row shifts
//     from an LDS table two taps ahead (a scalar kernel-argument load there would share lgkmcnt with the fragment reads).
// Scope (cv4_plan refuses the rest): bf16, Cin in {32, 64} (one resident chunk), Cout in {32, 64}, unit strides, whole
// lattice, zero padding, taps along one axis, 0 <= in_slope <= 1, LDS for weights + two halo stages.
// On gfx950 stores count in vmcnt together with the LDS-DMA pieces and the two kinds retire out of order with respect to
// each other: the wait at a tile boundary is vmcnt(0) (halo of this tile AND the stores of the previous one).
struct Cv4Params {
    int XR, npw;             // staged halo rows per tile (a multiple of 4 DMA instructions), x-DMA instructions per wave and tile
    int nwq;                 // weight DMA instructions (all taps)
    int tilesPerImg, totalTiles;
    int Pin, Pout, offmin;
    int toff[MSMC_CONV_MAX_TAPS];   // off[t] - offmin: row shift of tap t inside the halo tile
};
#define CV4_TM 128

template <int NCB, int CKM, bool DEFER>
MSMC_DEV void cv4_body(const msmc_conv_desc& d, const Cv4Params& P, const int wg, const int nwg) {
    MSMC_DYN_LDS(smem);
    typedef unsigned short T;
    constexpr int CK = 32 * CKM, CKV = CK / 8, KS = CK / 16, BN = 32 * NCB, RPI = 64 / CKV, R = 1 + NCB;
    int* taprow = (int*)smem;                                    // [32] halo-tile row shift of tap t
    T* wbuf = (T*)(smem + 128);                                  // [ntaps][BN][CK], source-swizzled rows
    const int wrows = d.ntaps * BN;
    T* ring = wbuf + (size_t)wrows * CK;                         // two stages of XR halo rows
    const int stage = P.XR * CK;
    const int tid = threadIdx.x, w = wave_uniform(tid >> 6), lane = tid & 63, i = lane & 31, g = lane >> 5;
    const int lrow = lane / CKV, pc = lane - lrow * CKV;         // row inside a DMA instruction, 16-byte piece of the row

    // ---- weights: once per workgroup (issued first: every later wait retires them too)
    {
        const T* wgl = (const T*)d.w;
        for (int q = w; q < P.nwq; q += 4) {
            const int row0 = q * RPI;
            const int t = wave_uniform(row0 / BN);
            const int n = row0 - t * BN + lrow;
            const T* src = wgl + ((size_t)d.tap_w[t] * d.Cout + n) * d.Cin + ((pc ^ cv3_key<CKM>(n)) * 8);
            lds_dma16(src, wbuf + (size_t)q * 512);
        }
    }
    if (tid < 32) taprow[tid] = tid < d.ntaps ? P.toff[tid] : 0;

    // ---- halo tile of one pixel tile: instruction q = w + 4k covers RPI rows
    const T* xbase = (const T*)d.x;
    auto issue_x = [&](int tile, T* st) {
        const int b = tile / P.tilesPerImg;
        const int p0 = (tile - b * P.tilesPerImg) * CV4_TM;
        const T* xtile = xbase + ((ptrdiff_t)b * P.Pin + p0 + P.offmin) * d.Cin;
        for (int k = 0; k < P.npw; ++k) {
            const int q = w + 4 * k;
            const int r = q * RPI + lrow, ip = p0 + P.offmin + r;
            const void* src = (const void*)msmc_cv3_zero_chunk;
            if (ip >= 0 && ip < P.Pin) src = xtile + (ptrdiff_t)r * d.Cin + ((pc ^ cv3_key<CKM>(r)) * 8);
            lds_dma16(src, st + (size_t)q * 512);
        }
    };

    // ---- fragment addressing: this wave's 32 pixels of the tile, every output-channel block
    const int prow = 32 * w + i;
    int arow[NCB], akey[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
        arow[cb] = (32 * cb + i) * CK;
        akey[cb] = cv3_key<CKM>(32 * cb + i);
    }
    f32x16 acc[NCB];
    auto load_frags = [&](const T* xt, int trow, int t, int ks, bf16x8 (&a)[NCB], bf16x8& bfr) {
        const int row = prow + trow;
        bfr = __builtin_bit_cast(bf16x8, lds_read128_async(xt + row * CK + (((2 * ks + g) ^ cv3_key<CKM>(row)) * 8)));
        const T* wb = wbuf + (size_t)t * BN * CK;
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
            a[cb] = __builtin_bit_cast(bf16x8, lds_read128_async(wb + arow[cb] + (((2 * ks + g) ^ akey[cb]) * 8)));
    };
    auto mma_frags = [&](bf16x8 (&a)[NCB], bf16x8& bfr) {
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) acc[cb] = mfma_bf16_32x32x16(a[cb], bfr, acc[cb]);
        sched_fence();
    };
    const int nt_ = d.ntaps;
    auto compute = [&](const T* xt) {
        bf16x8 a0[NCB], a1[NCB], b0, b1;
        int tr_cur = lds_read32_async(taprow), tr_nxt = lds_read32_async(taprow + 1);
        lds_wait<0>();
        load_frags(xt, tr_cur, 0, 0, a0, b0);
        for (int t = 0; t < nt_; ++t) {
            const int tr_n2 = lds_read32_async(taprow + ((t + 2) & 31));
            const int tn = t + 1 < nt_ ? t + 1 : t;              // the step after the last tap re-reads it and is never used
#pragma unroll
            for (int ks = 0; ks < KS; ks += 2) {
                load_frags(xt, tr_cur, t, ks + 1, a1, b1);
                if (ks == 0) lds_wait<R + 1>(); else lds_wait<R>();
                mma_frags(a0, b0);
                if (ks + 2 < KS) load_frags(xt, tr_cur, t, ks + 2, a0, b0);
                else load_frags(xt, t + 1 < nt_ ? tr_nxt : tr_cur, tn, 0, a0, b0);
                lds_wait<R>();
                mma_frags(a1, b1);
            }
            tr_cur = tr_nxt;
            tr_nxt = tr_n2;
        }
        lds_wait<0>();                                           // drain the unused last prefetch before its registers die
    };

    // ---- epilogue operands: a work-item owns channels 32*cb + 8*q4 + 4*g + (0..3) of one pixel
    const T* mask = (const T*)d.mask_src;
    const T* res = (const T*)d.res;
    const T* res2 = (const T*)d.res2;
    T* out = (T*)d.out;
    const float slope = d.in_slope, mslope = d.mask_slope, odiv = d.out_div, oslope = d.out_slope;
    float bv[NCB][16];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) bv[cb][r] = d.bias ? d.bias[32 * cb + 8 * (r >> 2) + 4 * g + (r & 3)] : 0.f;

    // DEFER (variant 33): the epilogue of a tile is issued in the NEXT iteration, after the wait / barrier / halo request --
    // what the next vmcnt(0) retires (halo, stores, operands) has then had a whole MFMA phase to complete
    u32x2 dmk[NCB][4], dr1[NCB][4], dr2[NCB][4];
    size_t dprev_o = 0;
    bool dprev_live = false, dhave = false;
    auto finish = [&](const size_t o, u32x2 (&mk)[NCB][4], u32x2 (&r1)[NCB][4], u32x2 (&r2)[NCB][4]) {
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
            {
                // all sixteen values of the channel block at once (cv_ep, conv.hip: one wave-uniform branch per optional operand)
                float ov[16];
                unsigned int mkw[8], r1w[8], r2w[8];
#pragma unroll
                for (int r = 0; r < 16; ++r) ov[r] = acc[cb][r] + bv[cb][r];
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    mkw[2 * q4] = mk[cb][q4][0]; mkw[2 * q4 + 1] = mk[cb][q4][1];
                    r1w[2 * q4] = r1[cb][q4][0]; r1w[2 * q4 + 1] = r1[cb][q4][1];
                    r2w[2 * q4] = r2[cb][q4][0]; r2w[2 * q4 + 1] = r2[cb][q4][1];
                }
                cv_ep<16>(ov, mkw, r1w, r2w, mask != nullptr, res != nullptr, res2 != nullptr, mslope, odiv, oslope);
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    const u32x2 pk = {pack_bf16x2(ov[4 * q4], ov[4 * q4 + 1]), pack_bf16x2(ov[4 * q4 + 2], ov[4 * q4 + 3])};
                    *(u32x2*)(out + o + 32 * cb + 8 * q4) = pk;
                }
            }
        }
    };
    auto pin_all = [&](u32x2 (&mk)[NCB][4], u32x2 (&r1)[NCB][4], u32x2 (&r2)[NCB][4]) {
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                vm_pin(mk[cb][q4]);
                vm_pin(r1[cb][q4]);
                vm_pin(r2[cb][q4]);
            }
    };

    if (wg < P.totalTiles) issue_x(wg, ring);
    int cur = 0;
    for (int tile = wg; tile < P.totalTiles; tile += nwg) {
        lds_dma_wait();                                          // this tile's halo (and the previous tile's stores)
        block_sync_lds();
        if (tile + nwg < P.totalTiles) issue_x(tile + nwg, ring + (size_t)(cur ^ 1) * stage);
        T* xt = ring + (size_t)cur * stage;
        cur ^= 1;
        if (DEFER && dhave) {                                    // previous tile: operands landed with the wait above
            pin_all(dmk, dr1, dr2);
            if (dprev_live) finish(dprev_o, dmk, dr1, dr2);
        }
        if (slope != 1.f) {                                      // input activation in place on the landed rows
            for (int e = tid; e < P.XR * CKV; e += 256) {
                u32x4 v = *(const u32x4*)(xt + (size_t)e * 8);
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = bf16x2_leaky(v[q], slope);
                *(u32x4*)(xt + (size_t)e * 8) = v;
            }
            block_sync_lds();
        }
        // epilogue operands of this tile: requested BEFORE the MFMA phase (their latency rides under it) by hand-counted
        // loads (global_load8_async: an ordinary load here would make hipcc drain the ring right after its request)
        const int b = tile / P.tilesPerImg;
        const int p = (tile - b * P.tilesPerImg) * CV4_TM + prow;
        const bool live = p < P.Pout;
        const size_t o = ((size_t)b * P.Pout + (live ? p : 0)) * d.Cout + 4 * g;
        if (DEFER) {
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    const u32x2 z = {0u, 0u};
                    dmk[cb][q4] = dr1[cb][q4] = dr2[cb][q4] = z;
                    if (mask && live) dmk[cb][q4] = global_load8_async(mask + o + 32 * cb + 8 * q4);
                    if (res && live) dr1[cb][q4] = global_load8_async(res + o + 32 * cb + 8 * q4);
                    if (res2 && live) dr2[cb][q4] = global_load8_async(res2 + o + 32 * cb + 8 * q4);
                }
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[cb][r] = 0.f;
            compute(xt);
            dprev_o = o;
            dprev_live = live;
            dhave = true;
            continue;
        }
        u32x2 mk[NCB][4], r1[NCB][4], r2[NCB][4];
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const u32x2 z = {0u, 0u};
                mk[cb][q4] = r1[cb][q4] = r2[cb][q4] = z;
            }
        if (mask && live) {
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) mk[cb][q4] = global_load8_async(mask + o + 32 * cb + 8 * q4);
        }
        if (res && live) {
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) r1[cb][q4] = global_load8_async(res + o + 32 * cb + 8 * q4);
        }
        if (res2 && live) {
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) r2[cb][q4] = global_load8_async(res2 + o + 32 * cb + 8 * q4);
        }
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[cb][r] = 0.f;
        compute(xt);
        if (mask || res || res2) {                               // the hand-counted operand loads (and the next halo tile)
            lds_dma_wait();
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    vm_pin(mk[cb][q4]);
                    vm_pin(r1[cb][q4]);
                    vm_pin(r2[cb][q4]);
                }
        }

        if (live) {
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) {
                {
                    // all sixteen values of the channel block at once (cv_ep, conv.hip: one wave-uniform branch per optional operand)
                    float ov[16];
                    unsigned int mkw[8], r1w[8], r2w[8];
#pragma unroll
                    for (int r = 0; r < 16; ++r) ov[r] = acc[cb][r] + bv[cb][r];
#pragma unroll
                    for (int q4 = 0; q4 < 4; ++q4) {
                        mkw[2 * q4] = mk[cb][q4][0]; mkw[2 * q4 + 1] = mk[cb][q4][1];
                        r1w[2 * q4] = r1[cb][q4][0]; r1w[2 * q4 + 1] = r1[cb][q4][1];
                        r2w[2 * q4] = r2[cb][q4][0]; r2w[2 * q4 + 1] = r2[cb][q4][1];
                    }
                    cv_ep<16>(ov, mkw, r1w, r2w, mask != nullptr, res != nullptr, res2 != nullptr, mslope, odiv, oslope);
#pragma unroll
                    for (int q4 = 0; q4 < 4; ++q4) {
                        const u32x2 pk = {pack_bf16x2(ov[4 * q4], ov[4 * q4 + 1]), pack_bf16x2(ov[4 * q4 + 2], ov[4 * q4 + 3])};
                        *(u32x2*)(out + o + 32 * cb + 8 * q4) = pk;
                    }
                }
            }
        }
    }
    if (DEFER && dhave) {                                        // the last tile of this workgroup
        lds_dma_wait();
        pin_all(dmk, dr1, dr2);
        if (dprev_live) finish(dprev_o, dmk, dr1, dr2);
    }
}

template <int NCB, int CKM>
__global__ __launch_bounds__(256, 2) void conv_gather4_kernel(msmc_conv_desc d, Cv4Params P) {
    cv4_body<NCB, CKM, false>(d, P, blockIdx.x, gridDim.x);
}
template <int NCB, int CKM>
__global__ __launch_bounds__(256, 2) void conv_gather4d_kernel(msmc_conv_desc d, Cv4Params P) {
    cv4_body<NCB, CKM, true>(d, P, blockIdx.x, gridDim.x);
}

// grouped form: the persistent grids of several members (the parallel ResBlocks of a generator stage) as one launch;
// member k owns workgroups [first[k], first[k+1]) and strides over ITS tiles with that many workgroups
struct Cv4GroupArgs {
    int n;
    int first[MSMC_GROUP_MAX + 1];
    msmc_conv_desc d[MSMC_GROUP_MAX];
    Cv4Params P[MSMC_GROUP_MAX];
};
template <int NCB, int CKM>
__global__ __launch_bounds__(256, 2) void conv_gather4_group_kernel(Cv4GroupArgs a) {
    const int k = cv_group_member(a.first, a.n);
    cv4_body<NCB, CKM, false>(a.d[k], a.P[k], blockIdx.x - a.first[k], a.first[k + 1] - a.first[k]);
}

struct Cv4Plan {
    int applies;
    int ncb, ckm;
    Cv4Params P;
    size_t lds;
    unsigned gx;
};

static bool cv4_is_variant(int variant) { return variant == 32 || variant == 33; }     // 33: deferred epilogue
static int msmc_cv4_grid_cap = 0;               // tests / sweeps: workgroups of the persistent grid (0 = one or two per CU)
extern "C" void msmc_conv_set_gather4_grid(int n) { msmc_cv4_grid_cap = n; }

static int cv4_plan(const msmc_conv_desc* d, Cv4Plan* pl) {
    pl->applies = 0;
    if (d->dtype != 1 || d->pad_mode != 0) return 0;
    if ((d->Cin != 32 && d->Cin != 64) || (d->Cout != 32 && d->Cout != 64)) return 0;
    if (d->ntaps <= 0 || d->ntaps > MSMC_CONV_MAX_TAPS) return 0;
    if (!(d->in_slope >= 0.f && d->in_slope <= 1.f)) return 0;
    if (d->isy != 1 || d->isx != 1 || d->osy != 1 || d->osx != 1 || d->oy0 || d->ox0 || d->QH != d->Hout ||
        d->QW != d->Wout)
        return 0;
    if ((((size_t)d->x) | ((size_t)d->w) | ((size_t)d->out) | ((size_t)d->res) | ((size_t)d->res2) | ((size_t)d->mask_src)) & 15)
        return 0;
    bool along_w = d->Hin == 1 && d->Hout == 1 && d->iy0 == 0, along_h = d->Win == d->Wout && d->ix0 == 0;
    for (int t = 0; t < d->ntaps; ++t) {
        if (d->tap_dy[t] != 0) along_w = false;
        if (d->tap_dx[t] != 0) along_h = false;
    }
    if (!along_w && !along_h) return 0;
    if ((long)d->B * d->Hin * d->Win * d->Cin >= (1L << 40)) return 0;
    Cv4Params& P = pl->P;
    P.Pin = d->Hin * d->Win;
    P.Pout = d->Hout * d->Wout;
    int off[MSMC_CONV_MAX_TAPS], offmin = 0, offmax = 0;
    for (int t = 0; t < d->ntaps; ++t) {
        off[t] = (d->iy0 + d->tap_dy[t]) * d->Win + d->ix0 + d->tap_dx[t];
        if (t == 0 || off[t] < offmin) offmin = off[t];
        if (t == 0 || off[t] > offmax) offmax = off[t];
    }
    const int span = offmax - offmin;
    if (span > 512) return 0;
    P.offmin = offmin;
    for (int t = 0; t < MSMC_CONV_MAX_TAPS; ++t) P.toff[t] = t < d->ntaps ? off[t] - offmin : 0;
    const int ckm = d->Cin / 32, ckv = d->Cin / 8, rpi = 64 / ckv;
    const int rows = CV4_TM + span;
    const int ninstr = ((rows + rpi - 1) / rpi + 3) & ~3;        // a multiple of the four waves
    P.XR = ninstr * rpi;
    P.npw = ninstr / 4;
    P.nwq = d->ntaps * d->Cout / rpi;
    P.tilesPerImg = (P.Pout + CV4_TM - 1) / CV4_TM;
    P.totalTiles = P.tilesPerImg * d->B;
    const size_t wbytes = (size_t)d->ntaps * d->Cout * d->Cin * 2, xbytes = (size_t)P.XR * d->Cin * 2;
    pl->lds = 128 + wbytes + 2 * xbytes;
    if (pl->lds > 160 * 1024) return 0;
    const int per_cu = pl->lds <= 80 * 1024 ? 2 : 1;
    int gx = per_cu * MSMC_NUM_CU;
    if (msmc_cv4_grid_cap > 0) gx = msmc_cv4_grid_cap;
    if (gx > P.totalTiles) gx = P.totalTiles;
    pl->gx = (unsigned)gx;
    pl->ncb = d->Cout / 32;
    pl->ckm = ckm;
    pl->applies = 1;
    return 0;
}

// one descriptor on the fourth generation: 1 = launched, 0 = does not apply, < 0 error
static int cv4_launch(const msmc_conv_desc* d, msmc_stream stream) {
    Cv4Plan pl;
    int rc = cv4_plan(d, &pl);
    if (rc) return rc;
    if (!pl.applies) return 0;
    const dim3 grid(pl.gx);
#define CV4_GO(NCB_, CKM_)                                                                                      \
    do {                                                                                                        \
        if (d->variant == 33) {                                                                                 \
            rc = msmc_allow_lds((const void*)conv_gather4d_kernel<NCB_, CKM_>, (int)pl.lds);               \
            if (rc) return rc < 0 ? rc : -rc;                                                                   \
            MSMC_LAUNCH((conv_gather4d_kernel<NCB_, CKM_>), grid, dim3(256), pl.lds, (msmc_stream_t)stream, *d, pl.P); \
        } else {                                                                                                \
            rc = msmc_allow_lds((const void*)conv_gather4_kernel<NCB_, CKM_>, (int)pl.lds);              \
            if (rc) return rc < 0 ? rc : -rc;                                                                   \
            MSMC_LAUNCH((conv_gather4_kernel<NCB_, CKM_>), grid, dim3(256), pl.lds, (msmc_stream_t)stream, *d, pl.P); \
        }                                                                                                       \
    } while (0)
    if (pl.ncb == 2 && pl.ckm == 2) CV4_GO(2, 2);
    else if (pl.ncb == 2) CV4_GO(2, 1);
    else if (pl.ckm == 2) CV4_GO(1, 2);
    else CV4_GO(1, 1);
#undef CV4_GO
    static thread_local char name[64];
    snprintf(name, sizeof(name), "%s<%d, %d>", d->variant == 33 ? "conv_gather4d_kernel" : "conv_gather4_kernel", pl.ncb, pl.ckm);
    msmc_conv_last = msmc_prof_name(name);
    return cv_launched(msmc_check_launch());
}

// Variant-32 members of a grouped call on ONE persistent grid (off by default: not yet timed on the GPU --
// msmc_conv_set_gather4_grouping(1) turns it on for sweeps).  done[i] is set for the members launched here.
static int msmc_cv4_grouping = 0;
extern "C" void msmc_conv_set_gather4_grouping(int on) { msmc_cv4_grouping = on; }
static int cv4_group_launch(const msmc_conv_desc* descs, int n, msmc_stream stream, bool* done) {
    Cv4Plan pl[MSMC_GROUP_LIMIT];
    bool mine[MSMC_GROUP_LIMIT];
    int count = 0;
    for (int i = 0; i < n; ++i) {
        mine[i] = false;
        if (!msmc_cv4_grouping || descs[i].variant != 32) continue;
        int rc = cv4_plan(&descs[i], &pl[i]);
        if (rc) return rc;
        mine[i] = pl[i].applies != 0;
        if (mine[i]) ++count;
    }
    if (count < 2) return 0;
    for (int i = 0; i < n; ++i) {
        if (!mine[i]) continue;
        Cv4GroupArgs a;
        a.n = 0;
        size_t lds = 0;
        int members[MSMC_GROUP_MAX];
        for (int j = i; j < n && a.n < MSMC_GROUP_MAX; ++j) {
            if (!mine[j] || pl[j].ncb != pl[i].ncb || pl[j].ckm != pl[i].ckm) continue;
            members[a.n++] = j;
            if (pl[j].lds > lds) lds = pl[j].lds;
        }
        if (a.n < 2) continue;                                   // a lone configuration goes the single-launch way
        // the chip's workgroup slots (one or two per CU, by the largest member) shared in proportion to the tile counts
        const int slots = msmc_cv4_grid_cap > 0 ? msmc_cv4_grid_cap : (lds <= 80 * 1024 ? 2 : 1) * MSMC_NUM_CU;
        long tiles = 0;
        for (int k = 0; k < a.n; ++k) tiles += pl[members[k]].P.totalTiles;
        int blocks = 0;
        for (int k = 0; k < a.n; ++k) {
            const int j = members[k];
            long share = tiles > slots ? ((long)pl[j].P.totalTiles * slots + tiles - 1) / tiles : pl[j].P.totalTiles;
            if (share < 1) share = 1;
            if (share > pl[j].P.totalTiles) share = pl[j].P.totalTiles;
            a.first[k] = blocks;
            a.d[k] = descs[j];
            a.P[k] = pl[j].P;
            blocks += (int)share;
            mine[j] = false;
            done[j] = true;
        }
        a.first[a.n] = blocks;
        ++msmc_conv_launches;
        int rc;
        const dim3 grid((unsigned)blocks);
#define CV4G_GO(NCB_, CKM_)                                                                                     \
    do {                                                                                                        \
        rc = msmc_allow_lds((const void*)conv_gather4_group_kernel<NCB_, CKM_>, (int)lds);                      \
        if (rc) return rc;                                                                                      \
        MSMC_LAUNCH((conv_gather4_group_kernel<NCB_, CKM_>), grid, dim3(256), lds, (msmc_stream_t)stream, a);   \
    } while (0)
        if (pl[i].ncb == 2 && pl[i].ckm == 2) CV4G_GO(2, 2);
        else if (pl[i].ncb == 2) CV4G_GO(2, 1);
        else if (pl[i].ckm == 2) CV4G_GO(1, 2);
        else CV4G_GO(1, 1);
#undef CV4G_GO
        static thread_local char name[64];
        snprintf(name, sizeof(name), "conv_gather4_group_kernel<%d, %d>", pl[i].ncb, pl[i].ckm);
        msmc_conv_last = msmc_prof_name(name);
        rc = msmc_check_launch();
        if (rc) return rc;
    }
    return 0;
}
