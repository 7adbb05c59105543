// wgrad4.inc -- fourth-generation bf16 weight gradient (included by conv_wgrad.hip after the second / third generation).
//
// Same result contract as the third generation (split partial results in a workspace, summed in split order by
// conv_wgrad_reduce_kernel; one split accumulates straight into dW), different operand movement.  Generations 2 / 3
// stage every pixel tile global -> registers -> LDS between two barriers, so a workgroup alternates between waiting
// for memory and feeding the matrix cores, and only the OTHER resident workgroup of the CU hides the load latency.
// Here the tiles of the workgroup's pixel range flow through a ring of NS stages filled by LDS-DMA
// (global_load_lds_dwordx4: no registers, no ds_write pass): while the matrix cores work on tile i, tiles i+1 ..
// i+NS-2 are in flight, ONE barrier per tile.
//
// Scope (wg4_plan refuses the rest, the caller falls back): bf16, unit strides, zero padding, whole-lattice output,
// Cin and Cout multiples of 8 (channel tiles of 64: the 16-byte pieces past the last channel read the zero chunk and their
// rows / columns of dW are not stored), no gradient mask, and taps that move along ONE axis only -- 1-D signals (H = 1) or
// k x 1 taps over [H][W] images of equal width (the period discriminators).  Both flatten to one pixel axis per
// image with  input pixel = output pixel + off[t],  zero outside [0, Pin): the x tile of TM output pixels is the
// contiguous row range [p0 + offmin, p0 + offmax + TM) and a tap is a row shift inside it.
//
// LDS image of a stage: TM rows of the output gradient, then XR rows of x, 64 channels (128 bytes) each.  The DMA
// image is lane-linear (eight rows per wave instruction), so the bank spread of the transposing fragment reads comes
// from the SOURCE permutation: rows with bit 1 set hold their two 64-byte halves swapped (four consecutive rows x
// 64 bytes then cover all 64 banks once).  Pixels outside the image read a 16-byte zero chunk.  The input leaky-ReLU
// (in_slope != 1) is applied to the x rows in place once the tile has landed.
struct Wg4Params {
    float* ws;               // per-split partial results [nsplit][ws_stride] (dW then db), NULL = one split, direct
    long ws_stride;
    int direct;
    int TM, XR, NS, npw;     // output pixels / staged x rows per tile, ring stages, LDS-DMA instructions per wave and tile
    int tilesPerWg, totalTiles, tilesPerImg;
    int TG, ntg;             // taps per workgroup, tap groups
    int Pin, Pout;           // pixels per image (flattened)
    int offmin;              // smallest tap offset
    int ablate;              // DIAGNOSTICS, 0 in production: 1 skip the MFMA steps, 2 skip the LDS-DMA (results are garbage)
    int toff[MSMC_CONV_MAX_TAPS];   // off[t] - offmin: row shift of tap t inside the x tile
};

static int msmc_wg4_ablate = 0;
extern "C" void msmc_conv_set_wgrad4_ablate(int mask) { msmc_wg4_ablate = mask; }

__device__ const u32x4 msmc_wg4_zero_chunk[1] = {{0u, 0u, 0u, 0u}};

// at most n LDS-DMA pieces of the calling wave still in flight (pieces land in issue order)
MSMC_DEV void wg4_dma_wait(int n) {
    switch (n) {
#define WG4_W(k) case k: lds_dma_wait_n<k>(); break;
        WG4_W(1) WG4_W(2) WG4_W(3) WG4_W(4) WG4_W(5) WG4_W(6) WG4_W(7) WG4_W(8) WG4_W(9) WG4_W(10) WG4_W(11) WG4_W(12)
        WG4_W(13) WG4_W(14) WG4_W(15) WG4_W(16) WG4_W(17) WG4_W(18) WG4_W(19) WG4_W(20) WG4_W(21) WG4_W(22) WG4_W(23)
        WG4_W(24) WG4_W(25) WG4_W(26) WG4_W(27) WG4_W(28) WG4_W(29) WG4_W(30) WG4_W(31) WG4_W(32)
#undef WG4_W
        default: lds_dma_wait_n<0>(); break;      // 0, or more than the table holds: waiting for everything is always safe
    }
}

// NKS 16-pixel steps of one tile: one A fragment (output gradient) and TPW B fragments (x rows shifted by the unit's
// tap) per step.  Units past the workgroup's tap range compute on the rows of shift 0 and are never stored.
// Software pipeline in source order: the 2 * (1 + TPW) transposing reads of step ks+1 are in flight under the MFMAs of
// step ks (hand-counted reads: hipcc otherwise sinks every read to its use and waits with lgkmcnt(0) per MFMA).
struct Wg4Frag {
    u32x2 lo, hi;
};
template <int KS>
MSMC_DEV Wg4Frag wg4_read(const unsigned short* p) {
    Wg4Frag f;
    f.lo = lds_read_tr16_async<KS * 2048>(p);
    f.hi = lds_read_tr16_async<KS * 2048 + 512>(p);
    return f;
}
MSMC_DEV bf16x8 wg4_frag(const Wg4Frag& f) {
    const u32x4 v = {f.lo[0], f.lo[1], f.hi[0], f.hi[1]};
    return __builtin_bit_cast(bf16x8, v);
}
// D = prefetch distance of the fragment reads in steps (a kernel template parameter: variant 4 runs D = 2 where the
// fragments fit the register budget of two waves per SIMD, variants 5 / 6 run D = 1; the host layer times both)
template <int KS, int NKS, int TPW, bool BIAS, int D>
struct Wg4Step {
    // (a, b) = step KS, (a1, b1) = step KS+1 (requested already when D == 2); this step requests KS+D
    static MSMC_DEV_INLINE void run(const unsigned short* ap, const unsigned short* const (&bp)[TPW], const Wg4Frag& a,
                                    const Wg4Frag (&b)[TPW], const Wg4Frag& a1, const Wg4Frag (&b1)[TPW],
                                    f32x16 (&acc)[TPW], float& bsum) {
        constexpr int NN = KS + D < NKS ? KS + D : 0;
        constexpr int younger = NKS - 1 - KS < D ? NKS - 1 - KS : D;      // steps requested after this one
        Wg4Frag an, bn[TPW];
        if (KS + D < NKS) {
            an = wg4_read<NN>(ap);
#pragma unroll
            for (int j = 0; j < TPW; ++j) bn[j] = wg4_read<NN>(bp[j]);
        }
        // (the LDS counter has four bits: at most 15 reads are tracked, so with three or four units the wait also retires
        //  the first reads of the next step -- conservative, never early)
        lds_wait<(2 * (1 + TPW) * younger > 15 ? 15 : 2 * (1 + TPW) * younger)>();
        const bf16x8 af = wg4_frag(a);
        if (BIAS) {
            const u16x8 ab = __builtin_bit_cast(u16x8, af);
#pragma unroll
            for (int q = 0; q < 8; ++q) bsum = bsum + bf16_bits_to_f32(ab[q]);
        }
#pragma unroll
        for (int j = 0; j < TPW; ++j) acc[j] = mfma_bf16_32x32x16(af, wg4_frag(b[j]), acc[j]);
        if (KS + 1 < NKS) {
            constexpr int K1 = KS + 1 < NKS ? KS + 1 : NKS;
            if (D == 2) Wg4Step<K1, NKS, TPW, BIAS, D>::run(ap, bp, a1, b1, an, bn, acc, bsum);
            else Wg4Step<K1, NKS, TPW, BIAS, D>::run(ap, bp, an, bn, an, bn, acc, bsum);
        }
    }
};
template <int NKS, int TPW, bool BIAS, int D>
struct Wg4Step<NKS, NKS, TPW, BIAS, D> {
    static MSMC_DEV_INLINE void run(const unsigned short*, const unsigned short* const (&)[TPW], const Wg4Frag&,
                                    const Wg4Frag (&)[TPW], const Wg4Frag&, const Wg4Frag (&)[TPW], f32x16 (&)[TPW],
                                    float&) {}
};
template <int NKS, int TPW, bool BIAS, int D>
MSMC_DEV void wg4_steps(const unsigned short* gt, const unsigned short* xt, const int aoff, const int (&boff)[TPW],
                        f32x16 (&acc)[TPW], float& bsum) {
    const unsigned short* ap = gt + aoff;
    const unsigned short* bp[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j) bp[j] = xt + boff[j];
    Wg4Frag a = wg4_read<0>(ap), b[TPW], a1, b1[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j) b[j] = wg4_read<0>(bp[j]);
    if (D == 2 && NKS > 1) {
        a1 = wg4_read<(NKS > 1 ? 1 : 0)>(ap);
#pragma unroll
        for (int j = 0; j < TPW; ++j) b1[j] = wg4_read<(NKS > 1 ? 1 : 0)>(bp[j]);
    }
    Wg4Step<0, NKS, TPW, BIAS, D>::run(ap, bp, a, b, a1, b1, acc, bsum);
}
template <int TPW, bool BIAS, int D>
MSMC_DEV void wg4_tile(const int nks, const unsigned short* gt, const unsigned short* xt, const int aoff,
                       const int (&boff)[TPW], f32x16 (&acc)[TPW], float& bsum) {
    switch (nks) {                                  // straight-line code per step count
        case 4: wg4_steps<4, TPW, BIAS, D>(gt, xt, aoff, boff, acc, bsum); break;
        case 5: wg4_steps<5, TPW, BIAS, D>(gt, xt, aoff, boff, acc, bsum); break;
        case 6: wg4_steps<6, TPW, BIAS, D>(gt, xt, aoff, boff, acc, bsum); break;
        case 7: wg4_steps<7, TPW, BIAS, D>(gt, xt, aoff, boff, acc, bsum); break;
        default: wg4_steps<8, TPW, BIAS, D>(gt, xt, aoff, boff, acc, bsum); break;
    }
}

template <int TPW, int D>
MSMC_DEV void wg4_body(const msmc_conv_desc& d, const unsigned short* __restrict__ gptr, float* __restrict__ dw,
                       float* __restrict__ db, const Wg4Params& P, const int block_x, const int block_y,
                       const int block_z) {
    MSMC_DYN_LDS(smem);
    unsigned short* ring = (unsigned short*)smem;
    const int TM = P.TM, XR = P.XR, NS = P.NS;
    const int stage = (TM + XR) * 64;                            // elements per ring stage
    const int tid = threadIdx.x, w = wave_uniform(tid >> 6), lane = tid & 63, L = lane & 15, half = (lane >> 4) & 1;
    const int g = lane >> 5;
    const int co0 = block_y * 64;
    const int ciTile = block_z / P.ntg, tg = block_z - ciTile * P.ntg;
    const int ci0 = ciTile * 64;

    // ---- this wave's units: output-channel block cb, then (input-channel block, tap) pairs (as the second generation
    // with both channel tiles full: two waves per output-channel block)
    const int cb = w & 1, slot = w >> 1;
    const int tap0 = tg * P.TG;
    int ntl = d.ntaps - tap0;
    if (ntl > P.TG) ntl = P.TG;
    const int nunits = 2 * ntl;
    const int frow = 8 * g + (L >> 2);                           // row this lane addresses inside a 16-row step
    int boff[TPW], utap[TPW], uib[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        const int u = slot + 2 * j;
        utap[j] = -1; uib[j] = 0;
        boff[j] = frow * 64 + 16 * half + 4 * (L & 3);
        if (u < nunits) {
            const int ib = u & 1, t = tap0 + (u >> 1);
            const int row = frow + P.toff[t];
            utap[j] = t; uib[j] = ib;
            boff[j] = row * 64 + ((32 * ib + 16 * half + 4 * (L & 3)) ^ (((row >> 1) & 1) << 5));
        }
    }
    const int aoff = frow * 64 + ((32 * cb + 16 * half + 4 * (L & 3)) ^ (((frow >> 1) & 1) << 5));
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

    // ---- LDS-DMA of one tile: instruction q (eight 128-byte rows) of the stage image; wave w issues q = w, w+4, ...
    const unsigned short* xbase = (const unsigned short*)d.x + ci0;
    const unsigned short* gbase = gptr + co0;
    const int drow = lane >> 3;                                  // row of this lane inside an instruction
    const int dchunk = ((lane & 7) ^ (((drow >> 1) & 1) << 2)) * 8;   // SOURCE channel offset (halves swapped on rows 2, 3, 6, 7)
    const int gq = TM >> 3;
    // (tile base addresses are wave-uniform scalars; the per-lane part is computed once)
    const int glane = drow * d.Cout + dchunk, xlane = drow * d.Cin + dchunk;
    const bool gpiece = co0 + dchunk < d.Cout, xpiece = ci0 + dchunk < d.Cin;   // (last channel tile of a count that is not a multiple of 64)
    auto issue = [&](int tile, unsigned short* st) {
        const int b = tile / P.tilesPerImg;
        const int p0 = (tile - b * P.tilesPerImg) * TM;
        const unsigned short* gtile = gbase + ((size_t)b * P.Pout + p0) * d.Cout;
        const unsigned short* xtile = xbase + ((ptrdiff_t)b * P.Pin + p0 + P.offmin) * d.Cin;
        for (int k = 0; k < P.npw; ++k) {
            const int q = w + 4 * k;
            const void* src = (const void*)msmc_wg4_zero_chunk;
            if (q < gq) {
                if (gpiece && p0 + 8 * q + drow < P.Pout) src = gtile + (size_t)(8 * q) * d.Cout + glane;
            } else {
                const int r0 = 8 * (q - gq), ip = p0 + P.offmin + r0 + drow;
                if (xpiece && ip >= 0 && ip < P.Pin) src = xtile + (ptrdiff_t)r0 * d.Cin + xlane;
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
        unsigned short* xt = gt + TM * 64;
        if (++cur_s == NS) cur_s = 0;
        if (d.in_slope != 1.f) {                                 // input activation in place (zero rows stay zero)
            for (int e = tid; e < XR * 8; e += 256) {
                u32x4 v = *(const u32x4*)(xt + (size_t)e * 8);
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = bf16x2_leaky(v[q], d.in_slope);
                *(u32x4*)(xt + (size_t)e * 8) = v;
            }
            block_sync_lds();
        }
        if (!mfma_on) continue;
        if (bias_wave) wg4_tile<TPW, true, D>(nks, gt, xt, aoff, boff, acc, bsum);   // (one workgroup per channel tile and split)
        else wg4_tile<TPW, false, D>(nks, gt, xt, aoff, boff, acc, bsum);
    }

    if (bias_wave) {
        // lane (i, g) summed output channel 32*cb + i over the pixels 8g..8g+7 of every 16-pixel step
        bsum = bsum + wave_xor(bsum, 32);
        if (g == 0 && co0 + 32 * cb + (lane & 31) < d.Cout) {
            float* q = db + co0 + 32 * cb + (lane & 31);
            *q = partial ? bsum : *q + bsum;
        }
    }
    // D fragment: row (co) = 32*cb + (r&3) + 8*(r>>2) + 4*g, col (ci) = 32*ib + (lane & 31)
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        if (utap[j] < 0) continue;
        const int ci = ci0 + 32 * uib[j] + (lane & 31);
        if (ci >= d.Cin) continue;
        float* dst = dw + (size_t)d.tap_w[utap[j]] * d.Cout * d.Cin;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + 32 * cb + (r & 3) + 8 * (r >> 2) + 4 * g;
            if (co >= d.Cout) continue;
            float* q = dst + (size_t)co * d.Cin + ci;
            *q = partial ? acc[j][r] : *q + acc[j][r];
        }
    }
}

template <int TPW, int D>
__global__ __launch_bounds__(256, 2) void conv_wgrad4_kernel(msmc_conv_desc d, const unsigned short* __restrict__ gptr,
                                                            float* __restrict__ dw, float* __restrict__ db,
                                                            Wg4Params P) {
    wg4_body<TPW, D>(d, gptr, dw, db, P, blockIdx.x, blockIdx.y, blockIdx.z);
}

// grouped weight gradients (see conv_wgrad2_group_kernel): members flattened over their (split, co tile, ci tile x taps)
struct Wg4GroupArgs {
    int n;
    int first[MSMC_GROUP_MAX + 1];
    int nx[MSMC_GROUP_MAX], ny[MSMC_GROUP_MAX];
    const unsigned short* g[MSMC_GROUP_MAX];
    float* dw[MSMC_GROUP_MAX];
    float* db[MSMC_GROUP_MAX];
    msmc_conv_desc d[MSMC_GROUP_MAX];
    Wg4Params P[MSMC_GROUP_MAX];
};
template <int TPW, int D>
__global__ __launch_bounds__(256, 2) void conv_wgrad4_group_kernel(Wg4GroupArgs a) {
    const int k = cv_group_member(a.first, a.n);
    int id = blockIdx.x - a.first[k];
    const int bx = id % a.nx[k];
    id /= a.nx[k];
    wg4_body<TPW, D>(a.d[k], a.g[k], a.dw[k], a.db[k], a.P[k], bx, id % a.ny[k], id / a.ny[k]);
}

struct Wg4Plan {
    Wg4Params P;
    size_t lds;
    int tpw;
    unsigned gx, gy, gz;
    size_t ws_floats;
};

// flavour: 0 (variant 4) three-stage ring, fragment reads two steps ahead; 1 (variant 5) one step ahead; 2 (variant 6)
// two-stage ring, one step ahead
// share: members of the grid this plan joins (a grouped launch fills the chip with all of them together)
static int wg4_plan(const msmc_conv_desc* d, const void* g, Wg4Plan* pl, int flavour, int share = 1) {
    if (d->dtype != 1 || d->pad_mode != 0 || d->mask_slope != 1.f) return MSMC_E_SHAPE;
    if (!(d->in_slope >= 0.f && d->in_slope <= 1.f)) return MSMC_E_SHAPE;      // (the in-place pass computes max(x, slope * x))
    if ((d->Cin & 7) || (d->Cout & 7) || d->Cin < 64 || d->Cout < 64) return MSMC_E_SHAPE;    // (16-byte pieces; thin layers: wgrad6.inc)
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
    // pixel tile: 64 .. 128 output pixels, the step count that wastes the least of the image's last tile
    int best = 8;
    long bestPad = -1;
    for (int nk = 8; nk >= 4; --nk) {
        const long tiles = (P.Pout + 16 * nk - 1) / (16 * nk), pad = tiles * nk;
        if (bestPad < 0 || pad < bestPad) { bestPad = pad; best = nk; }
    }
    P.TM = 16 * best;
    P.XR = ((2 * P.TM + span + 31) & ~31) - P.TM;               // (TM + XR) / 8 instructions: a multiple of the 4 waves
    P.npw = (P.TM + P.XR) / 32;
    const size_t stage_bytes = (size_t)(P.TM + P.XR) * 128;
    P.NS = flavour == 2 ? 2 : 3;
    while (P.NS > 2 && P.NS * stage_bytes > 80 * 1024) --P.NS;   // two workgroups per CU
    if (P.NS * stage_bytes > 160 * 1024) return MSMC_E_SHAPE;
    pl->lds = P.NS * stage_bytes;
    int tgmax = msmc_wgrad_tpw_cap;                              // taps per workgroup = accumulators per wave
    if (tgmax < 1) tgmax = 1;
    if (tgmax > 5) tgmax = 5;
    P.ntg = (d->ntaps + tgmax - 1) / tgmax;
    P.TG = (d->ntaps + P.ntg - 1) / P.ntg;
    pl->tpw = P.TG;
    P.tilesPerImg = (P.Pout + P.TM - 1) / P.TM;
    P.totalTiles = P.tilesPerImg * d->B;
    const int coT = (d->Cout + 63) / 64, ciT = (d->Cin + 63) / 64;
    const int cols = coT * ciT * P.ntg;
    // the ring holds the CU to two workgroups: split the pixel reduction until ONE round of them fills the chip
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
    P.direct = nsplit == 1;
    P.ws_stride = stride;
    pl->ws_floats = nsplit > 1 ? (size_t)(nsplit + wg3_reduce_plan(n_dw + d->Cout, nsplit).groups) * stride : 0;
    pl->gx = (unsigned)nsplit;
    pl->gy = (unsigned)coT;
    pl->gz = (unsigned)(ciT * P.ntg);
    return 0;
}
