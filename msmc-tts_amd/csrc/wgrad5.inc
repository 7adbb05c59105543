// wgrad5.inc -- bf16 weight gradient on the GENERAL lattice with LDS-DMA staging (included by conv_wgrad.hip after wgrad4.inc).
//
// Descriptor variant 7 only, not a tuner candidate yet: checked on the kernel interpreter (tests/test_product_emu.py) and
// timed once on the GPU (profiles/r02_wgrad5_first_measurement.txt: correct, 15 % ahead of generation 3 on the stride-3
// period-discriminator layers).  It is the third generation's machine mapping (wg2_body: 2-D lattice tiles, table-driven
// fragment rows, split partials + fixed-order second stage) with the fourth generation's operand movement for the layers
// wgrad4.inc cannot take -- strided, 2-D and reflection-padded ones (the period / resolution discriminators, now the
// symbol with the most time): the halo patch and the output-gradient tile of the NEXT lattice tile travel global -> LDS by
// global_load_lds_dwordx4 (one source address per 16-byte piece, so strides, reflection and zero padding are address
// choices) into the second of two stages while the matrix cores work on the current one; one LDS-only barrier per tile.
// The image is lane-linear, 128-byte rows without padding and without a source swizzle in this first form: the
// transposing fragment reads see two-way bank conflicts.  Bias gradient from the A fragments, input leaky-ReLU as one
// in-place pass over the landed patch.  Scope: Cin, Cout multiples of 64, no gradient mask, 0 <= in_slope <= 1.
struct Wg5Params {
    float* ws;               // per-split partial results (dW then db), NULL = one split, direct accumulation
    long ws_stride;
    int TM, npix;            // lattice points per tile (multiple of 16), halo pixels per tile
    int nq_x, nq_g, npw;     // LDS-DMA instructions of the halo patch / the gradient tile, per wave and tile (both)
    int tilesPerWg, totalTiles;
    int TG, ntg;
};

template <int TPW>
MSMC_DEV void wg5_body(const msmc_conv_desc& d, const unsigned short* __restrict__ gptr, float* __restrict__ dw,
                       float* __restrict__ db, const CvGeom& G, const Wg5Params& P, const int block_x, const int block_y,
                       const int block_z) {
    MSMC_DYN_LDS(smem);
    const int npix = P.npix, TM = P.TM;
    const int xrows = P.nq_x * 8, grows = P.nq_g * 8;            // staged rows (whole instructions)
    const int stage = (xrows + grows) * 64;                      // elements per ring stage
    int* xmeta = (int*)smem;                                     // [xrows] (ry << 16) | rx, -1 past the patch
    int* gmeta = xmeta + xrows;                                  // [grows] (mty << 16) | mtx, -1 past the tile
    unsigned short* ring = (unsigned short*)(smem + ((((size_t)(xrows + grows) * sizeof(int)) + 15) & ~(size_t)15));
    const int tid = threadIdx.x, w = wave_uniform(tid >> 6), lane = tid & 63, L = lane & 15, half = (lane >> 4) & 1;
    const int g = lane >> 5;
    const int co0 = block_y * 64;
    const int ciTile = block_z / P.ntg, tg = block_z - ciTile * P.ntg;
    const int ci0 = ciTile * 64;
    for (int pi = tid; pi < xrows; pi += 256) {
        const int ry = pi / G.IW;
        xmeta[pi] = pi < npix ? ((ry << 16) | (pi - ry * G.IW)) : -1;
    }
    for (int m = tid; m < grows; m += 256) {
        const int mty = m / G.TW;
        gmeta[m] = (m < TM && mty < G.TH) ? ((mty << 16) | (m - mty * G.TW)) : -1;
    }
    __syncthreads();

    // ---- this wave's units (both channel tiles are full): output-channel block cb, (input-channel block, tap) pairs
    const int cb = w & 1, slot = w >> 1;
    const int tap0 = tg * P.TG;
    int ntl = d.ntaps - tap0;
    if (ntl > P.TG) ntl = P.TG;
    const int nunits = 2 * ntl;
    int boff[TPW], utap[TPW], uib[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        const int u = slot + 2 * j;
        utap[j] = -1; uib[j] = 0; boff[j] = 0;
        if (u < nunits) {
            const int ib = u & 1, t = tap0 + (u >> 1);
            utap[j] = t; uib[j] = ib;
            boff[j] = ((d.tap_dy[t] - G.dyMin) * G.IW + (d.tap_dx[t] - G.dxMin)) * 64 + 32 * ib + 16 * half + 4 * (L & 3);
        }
    }
    const int acol = 32 * cb + 16 * half + 4 * (L & 3);
    int xrow[16];                                                // halo-patch row (x 64) of the lattice points this lane addresses
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = 16 * (r >> 1) + 8 * g + 4 * (r & 1) + (L >> 2);
        const int meta = m < grows ? gmeta[m] : -1;
        xrow[r] = meta >= 0 ? ((meta >> 16) * d.isy * G.IW + (meta & 0xffff) * d.isx) * 64 : 0;
    }
    f32x16 acc[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    const bool partial = P.ws != nullptr;
    if (partial) {
        dw = P.ws + (size_t)block_x * P.ws_stride;
        if (db) db = dw + (size_t)d.ntaps * d.Cout * d.Cin;
    }
    const bool bias_wave = (db != nullptr) && (block_z == 0) && (slot == 0);
    float bsum = 0.f;
    const int nks = TM >> 4;
    const int t0 = block_x * P.tilesPerWg;
    int t1 = t0 + P.tilesPerWg;
    if (t1 > P.totalTiles) t1 = P.totalTiles;

    // ---- LDS-DMA of one lattice tile: instructions 0 .. nq_x-1 = halo rows, nq_x .. nq_x+nq_g-1 = gradient rows
    const int drow = lane >> 3, dchunk = (lane & 7) * 8;
    auto issue = [&](int tile, unsigned short* st) {
        int bt = tile;
        const int tx_ = bt % G.tilesX;
        bt /= G.tilesX;
        const int ty_ = bt % G.tilesY;
        const int b = bt / G.tilesY;
        const int qy0 = ty_ * G.TH, qx0 = tx_ * G.TW;
        const int iyBase = qy0 * d.isy + d.iy0 + G.dyMin, ixBase = qx0 * d.isx + d.ix0 + G.dxMin;
        const unsigned short* xb = (const unsigned short*)d.x + (size_t)b * d.Hin * d.Win * d.Cin + ci0 + dchunk;
        const unsigned short* gb = gptr + (size_t)b * d.Hout * d.Wout * d.Cout + co0 + dchunk;
        for (int k = 0; k < P.npw; ++k) {
            const int q = w + 4 * k;
            const void* src = (const void*)msmc_wg4_zero_chunk;
            if (q < P.nq_x) {
                const int meta = xmeta[8 * q + drow];
                if (meta >= 0) {
                    int iy = iyBase + (meta >> 16), ix = ixBase + (meta & 0xffff);
                    bool inside = true;
                    if (d.pad_mode == 1) {
                        iy = reflect_index(iy, d.Hin);
                        ix = reflect_index(ix, d.Win);
                    } else {
                        inside = (iy >= 0) && (iy < d.Hin) && (ix >= 0) && (ix < d.Win);
                    }
                    if (inside) src = xb + ((size_t)iy * d.Win + ix) * d.Cin;
                }
            } else if (q < P.nq_x + P.nq_g) {
                const int meta = gmeta[8 * (q - P.nq_x) + drow];
                if (meta >= 0) {
                    const int qy = qy0 + (meta >> 16), qx = qx0 + (meta & 0xffff);
                    if (qy < d.QH && qx < d.QW) {
                        const int oy = d.oy0 + qy * d.osy, ox = d.ox0 + qx * d.osx;
                        src = gb + ((size_t)oy * d.Wout + ox) * d.Cout;
                    }
                }
            }
            if (q < P.nq_x + P.nq_g) lds_dma16(src, st + (size_t)q * 512);
        }
    };

    if (t0 < t1) issue(t0, ring);
    int cur = 0;
    for (int tile = t0; tile < t1; ++tile) {
        lds_dma_wait();                                          // this tile has landed
        block_sync_lds();                                        // ... for every wave, and the previous tile is consumed
        if (tile + 1 < t1) issue(tile + 1, ring + (size_t)(cur ^ 1) * stage);
        unsigned short* xt = ring + (size_t)cur * stage;
        unsigned short* gt = xt + (size_t)xrows * 64;
        cur ^= 1;
        if (d.in_slope != 1.f) {                                 // input activation in place (zero rows stay zero)
            for (int e = tid; e < xrows * 8; e += 256) {
                u32x4 v = *(const u32x4*)(xt + (size_t)e * 8);
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = bf16x2_leaky(v[q], d.in_slope);
                *(u32x4*)(xt + (size_t)e * 8) = v;
            }
            block_sync_lds();
        }
        if (utap[0] < 0) continue;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            if (ks >= nks) continue;
            const int m0 = 16 * ks + 8 * g + (L >> 2);
            const bf16x8 af = wg_frag(gt, 1, m0 * 64, (m0 + 4) * 64, acol);
            if (bias_wave) {
                const u16x8 ab = __builtin_bit_cast(u16x8, af);
#pragma unroll
                for (int q = 0; q < 8; ++q) bsum = bsum + bf16_bits_to_f32(ab[q]);
            }
#pragma unroll
            for (int j = 0; j < TPW; ++j) {
                if (utap[j] >= 0) {
                    const bf16x8 bf = wg_frag(xt, 1, xrow[2 * ks] + boff[j], xrow[2 * ks + 1] + boff[j], 0);
                    acc[j] = mfma_bf16_32x32x16(af, bf, acc[j]);
                }
            }
        }
    }

    if (bias_wave) {
        bsum = bsum + wave_xor(bsum, 32);
        if (g == 0) {
            float* q = db + co0 + 32 * cb + (lane & 31);
            *q = partial ? bsum : *q + bsum;
        }
    }
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        if (utap[j] < 0) continue;
        const int ci = ci0 + 32 * uib[j] + (lane & 31);
        float* dst = dw + (size_t)d.tap_w[utap[j]] * d.Cout * d.Cin;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + 32 * cb + (r & 3) + 8 * (r >> 2) + 4 * g;
            float* q = dst + (size_t)co * d.Cin + ci;
            *q = partial ? acc[j][r] : *q + acc[j][r];
        }
    }
}

template <int TPW>
__global__ __launch_bounds__(256, 2) void conv_wgrad5_kernel(msmc_conv_desc d, const unsigned short* __restrict__ gptr,
                                                            float* __restrict__ dw, float* __restrict__ db, CvGeom G,
                                                            Wg5Params P) {
    wg5_body<TPW>(d, gptr, dw, db, G, P, blockIdx.x, blockIdx.y, blockIdx.z);
}

// grouped form (see conv_wgrad4_group_kernel): members flattened over their (split, co tile, ci tile x taps)
struct Wg5GroupArgs {
    int n;
    int first[MSMC_GROUP_MAX + 1];
    int nx[MSMC_GROUP_MAX], ny[MSMC_GROUP_MAX];
    const unsigned short* g[MSMC_GROUP_MAX];
    float* dw[MSMC_GROUP_MAX];
    float* db[MSMC_GROUP_MAX];
    msmc_conv_desc d[MSMC_GROUP_MAX];
    CvGeom G[MSMC_GROUP_MAX];
    Wg5Params P[MSMC_GROUP_MAX];
};
template <int TPW>
__global__ __launch_bounds__(256, 2) void conv_wgrad5_group_kernel(Wg5GroupArgs a) {
    const int k = cv_group_member(a.first, a.n);
    int id = blockIdx.x - a.first[k];
    const int bx = id % a.nx[k];
    id /= a.nx[k];
    wg5_body<TPW>(a.d[k], a.g[k], a.dw[k], a.db[k], a.G[k], a.P[k], bx, id % a.ny[k], id / a.ny[k]);
}

struct Wg5Plan {
    Wg5Params P;
    CvGeom G;
    size_t lds;
    int tpw;
    unsigned gx, gy, gz;
    size_t ws_floats;
};

static int wg5_plan(const msmc_conv_desc* d, const void* g, Wg5Plan* pl, int share = 1) {
    if (d->dtype != 1 || d->mask_slope != 1.f || (d->Cin & 63) || (d->Cout & 63)) return MSMC_E_SHAPE;
    if (!(d->in_slope >= 0.f && d->in_slope <= 1.f)) return MSMC_E_SHAPE;
    if ((((size_t)d->x) | ((size_t)g)) & 15) return MSMC_E_SHAPE;
    Wg5Params& P = pl->P;
    P.ws = nullptr;
    CvGeom& G = pl->G;
    size_t lds_unused, lds = 0;
    int TM = WG_TM, rc;
    for (;;) {                                     // shrink the lattice tile until two workgroups (two stages each) fit a CU
        rc = cv_geometry(d, &G, 2, 64, 0, &lds_unused, TM);
        if (rc) return rc;
        TM = ((G.TH * G.TW + 15) / 16) * 16;
        P.npix = G.IH * G.IW;
        P.nq_x = (P.npix + 7) / 8;
        P.nq_g = (TM + 7) / 8;
        const size_t rows = (size_t)(P.nq_x + P.nq_g) * 8;
        lds = ((rows * sizeof(int) + 15) & ~(size_t)15) + 2 * rows * 128;
        if (lds <= 80 * 1024 && G.IH < 32768 && G.IW < 65536) break;
        if (G.TH * G.TW <= 16) {
            if (lds <= 160 * 1024) break;
            return MSMC_E_SHAPE;
        }
        TM = (G.TH * G.TW) / 2;
    }
    P.TM = TM;
    P.npw = (P.nq_x + P.nq_g + 3) / 4;
    pl->lds = lds;
    int tgmax = msmc_wgrad_tpw_cap;
    if (tgmax < 1) tgmax = 1;
    if (tgmax > 5) tgmax = 5;
    P.ntg = (d->ntaps + tgmax - 1) / tgmax;
    P.TG = (d->ntaps + P.ntg - 1) / P.ntg;
    pl->tpw = P.TG;
    P.totalTiles = G.tilesX * G.tilesY * d->B;
    const int cols = (d->Cout / 64) * (d->Cin / 64) * P.ntg;
    int nsplit = (2 * MSMC_NUM_CU) / (cols * (share > 1 ? share : 1));
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
    P.ws_stride = stride;
    pl->ws_floats = nsplit > 1 ? (size_t)(nsplit + wg3_reduce_plan(n_dw + d->Cout, nsplit).groups) * stride : 0;
    pl->gx = (unsigned)nsplit;
    pl->gy = (unsigned)(d->Cout / 64);
    pl->gz = (unsigned)((d->Cin / 64) * P.ntg);
    return 0;
}
