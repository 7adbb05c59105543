// gather3.inc -- third-generation bf16 forward / data-gradient implicit GEMM (included by conv.hip).
//
// Same descriptor semantics as conv_gather2_kernel (lattice + tap table + padding rule + input activation + epilogue),
// different machine mapping:
//   * a workgroup owns BM = 64*WM lattice points x BN = 32*NTW*(4/WM) output channels; each of its four waves owns a
//     64 x (32*NTW) sub-tile = 2 x NTW accumulators of v_mfma_f32_32x32x16_bf16, so every A fragment read from LDS
//     feeds NTW MFMAs and every B fragment two (gather2: one wave = 32 rows, every fragment feeds one MFMA);
//   * software pipeline over 64- or 128-byte channel chunks with ONE barrier per chunk: while the matrix cores work on
//     chunk c, the weight slices of chunk c+1 stream global -> LDS directly (global_load_lds_dwordx4: no registers,
//     no ds_write pass) into the second weight buffer, and the input halo tile of chunk c+1 sits in registers
//     (padding rule and input leaky-ReLU are applied on its way into the second halo buffer, after the MFMAs);
//   * the LDS-DMA image is lane-linear (destination = wave base + 16*lane), so bank conflicts of the B-fragment reads
//     are removed by permuting the SOURCE: 16-byte chunk c of weight row n lives at chunk c ^ key(n), and the
//     fragment read applies the same XOR (MI355X guide 5.4 rule 21).  The halo tile is written from registers, so
//     it keeps the padded row pitch.
//   * variants 24..31 (= 16..23 + 8): the halo tile travels by LDS-DMA as well (the fourth-generation weight gradient's
//     operand movement, wgrad4.inc): no staging registers, no ds_write pass.  Its image is lane-linear too (unpadded
//     rows of one chunk), so the A-fragment reads take the weight rows' XOR key on the halo pixel index; padding pixels
//     read a 16-byte zero chunk, reflected pixels their mirror image, and an input leaky-ReLU becomes one in-place pass
//     over the landed tile (one more barrier per chunk).
// Requirements (the planner falls back to the second generation otherwise): bf16, Cin a multiple of the chunk,
// halo tile of at most 12 vectors per work-item.
#define CV3_MAX_XV 12

__device__ const u32x4 msmc_cv3_zero_chunk[1] = {{0u, 0u, 0u, 0u}};

struct Cv3Plan {
    int applies;
    int wm, ntw, ckm, xv, xdma;
    CvGeom G;
    size_t lds;
    unsigned gx, gy;
};

template <int CKM>
MSMC_DEV int cv3_key(int n) {                       // XOR key of weight row n (16-byte chunk index within the row)
    return CKM == 1 ? ((n >> 2) & 3) : ((n >> 1) & 7);
}

template <int WM, int NTW, int CKM, int XV, bool XD>
MSMC_DEV void cv3_body(const msmc_conv_desc& d, const CvGeom& G, const int block_x, const int block_y) {
    MSMC_DYN_LDS(smem);
    typedef unsigned short T;
    constexpr int WN = 4 / WM, BM = 64 * WM, BNW = 32 * NTW, BN = BNW * WN;
    constexpr int CK = 32 * CKM, CKV = CK / 8, XS = CK + 8, OS = BN + 4, BNV = BN / 8;
    const int npix = G.IH * G.IW, IW = G.IW;
    int* in_off = (int*)smem;                                   // [npix] element offset of halo pixel, -1 = zero
    int* out_off = in_off + npix;                               // [BM]   pixel index of lattice point, -1 = none
    int* taprow = out_off + BM;                                 // [32]   halo-tile row (pixel) shift of tap t
    char* region = smem + (((size_t)(npix + BM + 32) * sizeof(int) + 15) & ~(size_t)15);
    constexpr bool xdma = XD;                                    // halo tile by LDS-DMA (unpadded, source-swizzled rows)
    const int xs = xdma ? CK : XS;                               // halo-tile row pitch (elements)
    const size_t xbytes = xdma ? ((((size_t)npix * CK * sizeof(T)) + 1023) & ~(size_t)1023)
                               : ((((size_t)npix * XS * sizeof(T)) + 15) & ~(size_t)15);
    const size_t wbytes = (size_t)d.ntaps * BN * CK * sizeof(T);
    T* xbuf0 = (T*)region;
    T* xbuf1 = (T*)(region + xbytes);
    T* wbuf0 = (T*)(region + 2 * xbytes);
    T* wbuf1 = (T*)(region + 2 * xbytes + wbytes);
    float* ot = (float*)region;                                 // [BM][OS] epilogue tile (aliases the staging buffers)

    const int tid = threadIdx.x, w = wave_uniform(tid >> 6), lane = tid & 63, i = lane & 31, g = lane >> 5;
    const int wm_ = w % WM, wn_ = w / WM;
    int bt = block_x;
    const int tx_ = bt % G.tilesX;
    bt /= G.tilesX;
    const int ty_ = bt % G.tilesY;
    const int b = bt / G.tilesY;
    const int co0 = block_y * BN;
    const int qy0 = ty_ * G.TH, qx0 = tx_ * G.TW;
    const int iyBase = qy0 * d.isy + d.iy0 + G.dyMin, ixBase = qx0 * d.isx + d.ix0 + G.dxMin;

    int arow[2], brow[NTW], bkey[NTW];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int m = 64 * wm_ + 32 * mt + i;
        const int mty = m / G.TW, mtx = m - mty * G.TW;
        arow[mt] = (mty < G.TH) ? (mty * d.isy) * IW + mtx * d.isx : 0;      // halo pixel of the lattice point at tap shift 0
    }
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
        const int n = wn_ * BNW + 32 * nt + i;
        brow[nt] = n * CK;
        bkey[nt] = cv3_key<CKM>(n);
    }
    f32x16 acc[2][NTW];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;

    const T* xb = (const T*)d.x + (size_t)b * d.Hin * d.Win * d.Cin;
    const T* wg = (const T*)d.w;
    const float slope = d.in_slope;
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    const int nxv = npix * CKV;
    const int nwq = d.ntaps * BN * CKV / 64;                    // LDS-DMA wave-instructions per chunk (64 vectors each)

    // weight slices of one chunk: global -> LDS, no registers; wave w issues instructions w, w+4, ...  One instruction
    // covers 64 / CKV consecutive rows of ONE tap (BN is a multiple of 16), so the tap is wave-uniform and its weight
    // slice comes from the kernel argument (no LDS table: the first chunk is issued before the tables exist).
    auto issue_w = [&](int c0, T* wbuf) {
        constexpr int RPI = 64 / CKV;                           // weight rows per instruction
        const int nl = lane / CKV, pc = lane - nl * CKV;        // row within the instruction, physical chunk in the LDS row
        for (int q = w; q < nwq; q += 4) {
            const int row0 = q * RPI;
            const int t = wave_uniform(row0 / BN);
            const int n = row0 - t * BN + nl;
            int co = co0 + n;
            if (co >= d.Cout) co = d.Cout - 1;                  // columns past Cout are never stored: any valid row
            const int lc = pc ^ cv3_key<CKM>(n);
            const T* src = wg + ((size_t)d.tap_w[t] * d.Cout + co) * d.Cin + c0 + lc * 8;
            lds_dma16(src, wbuf + (size_t)q * 512);
        }
    };
    auto load_x = [&](int c0, u32x4 (&regs)[XV]) {
#pragma unroll
        for (int u = 0; u < XV; ++u) {
            const int e = tid + 256 * u;
            regs[u] = zero4;
            if (e < nxv) {
                const int pi = e / CKV, v = e - pi * CKV;
                const int off = in_off[pi];
                if (off >= 0) regs[u] = *(const u32x4*)(xb + off + c0 + v * 8);
            }
        }
    };
    auto commit_x = [&](u32x4 (&regs)[XV], T* xbuf) {
#pragma unroll
        for (int u = 0; u < XV; ++u) {
            const int e = tid + 256 * u;
            if (e >= nxv) continue;
            const int pi = e / CKV, v = e - pi * CKV;
            u32x4 val = regs[u];
            if (slope != 1.f) {
                alignas(16) T tmp[8];
                *(u32x4*)tmp = val;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    float f = bf16_bits_to_f32(tmp[q]);
                    f = f > 0.f ? f : f * slope;
                    tmp[q] = f32_to_bf16_bits(f);
                }
                val = *(const u32x4*)tmp;
            }
            *(u32x4*)(xbuf + (size_t)pi * XS + v * 8) = val;
        }
    };
    // MFMA phase of one chunk: k16 steps s = (tap, 16-channel slice).  The fragments of step s+1 are in flight while
    // the MFMAs of step s issue (two register sets; KS is even, so a tap always starts on set 0); the halo-tile row
    // offset of a tap is read from its LDS table two taps ahead.  All LDS reads of this phase are hand-counted
    // (lds_read*_async / lds_wait<N>): R = 2 + NTW reads per fragment set, one table read at the top of a tap.
    constexpr int KS = CK / 16, R = 2 + NTW;
    auto load_frags = [&](const T* xbuf, const T* wbuf, int trow, int t, int ks, bf16x8 (&a)[2], bf16x8 (&bf)[NTW]) {
        const T* bb = wbuf + (size_t)t * BN * CK;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const int row = arow[mt] + trow;
            const int key = xdma ? cv3_key<CKM>(row) : 0;
            a[mt] = __builtin_bit_cast(bf16x8, lds_read128_async(xbuf + row * xs + (((2 * ks + g) ^ key) * 8)));
        }
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt)
            bf[nt] = __builtin_bit_cast(bf16x8, lds_read128_async(bb + brow[nt] + (((2 * ks + g) ^ bkey[nt]) * 8)));
    };
    auto mma_frags = [&](bf16x8 (&a)[2], bf16x8 (&bf)[NTW]) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) acc[mt][nt] = mfma_bf16_32x32x16(a[mt], bf[nt], acc[mt][nt]);
        sched_fence();
    };
    auto compute = [&](const T* xbuf, const T* wbuf) {
        const int nt_ = d.ntaps;
        bf16x8 a0[2], b0[NTW], a1[2], b1[NTW];
        int tr_cur = lds_read32_async(taprow), tr_nxt = lds_read32_async(taprow + 1);    // (32 entries: reads past ntaps are harmless)
        lds_wait<0>();
        load_frags(xbuf, wbuf, tr_cur, 0, 0, a0, b0);
        for (int t = 0; t < nt_; ++t) {
            // in flight here: set 0 of this tap (R reads)
            const int tr_n2 = lds_read32_async(taprow + t + 2);
            const int tn = t + 1 < nt_ ? t + 1 : t;             // the step after the last tap re-reads it and is never used
#pragma unroll
            for (int ks = 0; ks < KS; ks += 2) {
                load_frags(xbuf, wbuf, tr_cur, t, ks + 1, a1, b1);
                if (ks == 0) lds_wait<R + 1>(); else lds_wait<R>();            // set 0 landed (table read + set 1 may fly)
                mma_frags(a0, b0);
                if (ks + 2 < KS) load_frags(xbuf, wbuf, tr_cur, t, ks + 2, a0, b0);
                else load_frags(xbuf, wbuf, t + 1 < nt_ ? tr_nxt : tr_cur, tn, 0, a0, b0);
                lds_wait<R>();                                                  // set 1 (and the table read) landed
                mma_frags(a1, b1);
            }
            tr_cur = tr_nxt;
            tr_nxt = tr_n2;
        }
        lds_wait<0>();                                          // drain the unused last prefetch before its registers die
    };

    issue_w(0, wbuf0);                                          // in flight while the offset tables are built
    for (int pi = tid; pi < npix; pi += 256) {
        const int ry = pi / IW, rx = pi - ry * IW;
        int iy = iyBase + ry, ix = ixBase + rx;
        bool inside = true;
        if (d.pad_mode == 1) {
            iy = reflect_index(iy, d.Hin);
            ix = reflect_index(ix, d.Win);
        } else {
            inside = (iy >= 0) && (iy < d.Hin) && (ix >= 0) && (ix < d.Win);
        }
        in_off[pi] = inside ? (iy * d.Win + ix) * d.Cin : -1;
    }
    for (int m = tid; m < BM; m += 256) {
        const int mty = m / G.TW, mtx = m - mty * G.TW;
        const int qy = qy0 + mty, qx = qx0 + mtx;
        const bool valid = mty < G.TH && qy < d.QH && qx < d.QW;
        out_off[m] = valid ? (d.oy0 + qy * d.osy) * d.Wout + (d.ox0 + qx * d.osx) : -1;
    }
    if (tid < 32)
        taprow[tid] = tid < d.ntaps ? (d.tap_dy[tid] - G.dyMin) * IW + (d.tap_dx[tid] - G.dxMin) : 0;

    __syncthreads();                                            // offset tables ready
    const int nchunks = d.Cin / CK;
    // halo tile by LDS-DMA: instruction q = w + 4u covers 64 consecutive 16-byte pieces (64 / CKV pixels of one chunk);
    // this lane's piece of it is the same for every chunk: element offset in x (source-swizzled), -1 = zero chunk
    const int nxq = (nxv + 63) / 64;
    int xoff[XV];
    if (xdma) {
#pragma unroll
        for (int u = 0; u < XV; ++u) {
            const int e = (w + 4 * u) * 64 + lane;
            xoff[u] = -1;
            if (e < nxv) {
                const int pi = e / CKV, pc = e - pi * CKV;
                const int off = in_off[pi];
                if (off >= 0) xoff[u] = off + ((pc ^ cv3_key<CKM>(pi)) * 8);
            }
        }
    }
    auto issue_x = [&](int c0, T* xbuf) {
#pragma unroll
        for (int u = 0; u < XV; ++u) {
            const int q = w + 4 * u;
            if (q < nxq) {
                const void* src = xoff[u] >= 0 ? (const void*)(xb + xoff[u] + c0) : (const void*)msmc_cv3_zero_chunk;
                lds_dma16(src, xbuf + (size_t)q * 512);
            }
        }
    };
    const int abl0 = d.split_shift;
    if (xdma) {
        if (!(abl0 & 4)) issue_x(0, xbuf0);
    } else {
        u32x4 regs[XV];
        load_x(0, regs);
        commit_x(regs, xbuf0);
    }
    lds_dma_wait();
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        T* xcur = (c & 1) ? xbuf1 : xbuf0;
        T* xnxt = (c & 1) ? xbuf0 : xbuf1;
        T* wcur = (c & 1) ? wbuf1 : wbuf0;
        T* wnxt = (c & 1) ? wbuf0 : wbuf1;
        const bool more = c + 1 < nchunks;
        u32x4 regs[XV];
        const int abl = d.split_shift;                          // ABLATION (diagnostics): 1 no MFMA, 2 no weight stream, 4 no halo loads, 8 no epilogue
        if (xdma && slope != 1.f) {                             // input activation in place on the landed tile
            for (int e = tid; e < nxv; e += 256) {
                u32x4 v = *(const u32x4*)(xcur + (size_t)e * 8);
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = bf16x2_leaky(v[q], slope);
                *(u32x4*)(xcur + (size_t)e * 8) = v;
            }
            __syncthreads();
        }
        if (more) {
            if (!(abl & 2)) issue_w((c + 1) * CK, wnxt);
            if (!(abl & 4)) {
                if (xdma) issue_x((c + 1) * CK, xnxt);
                else load_x((c + 1) * CK, regs);
            }
        }
        if (!(abl & 1)) compute(xcur, wcur);
        if (more && !(abl & 4) && !xdma) commit_x(regs, xnxt);
        lds_dma_wait();
        __syncthreads();
    }

    // ---- epilogue: accumulators -> fp32 LDS tile -> 16-byte vectors of consecutive output channels
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                ot[(64 * wm_ + 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * g) * OS + wn_ * BNW + 32 * nt + i] = acc[mt][nt][r];
    __syncthreads();
    const T* mask = (const T*)d.mask_src;
    const T* res = (const T*)d.res;
    const T* res2 = (const T*)d.res2;
    T* out = (T*)d.out;
    const size_t img = (size_t)b * d.Hout * d.Wout;
    // a work-item owns ONE vector of 8 consecutive output channels and walks the rows: the bias vector is loaded once
    constexpr int RSTEP = 256 / BNV;                            // rows covered per pass of the workgroup
    const int vcol = (tid % BNV) * 8, co = co0 + vcol;
    if (co < d.Cout && !(d.split_shift & 8)) {
        const bool ovec = (d.Cout % 8) == 0;                    // then co + 7 < Cout
        float bv[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) bv[q] = (d.bias && co + q < d.Cout) ? d.bias[co + q] : 0.f;
        const float mslope = d.mask_slope, odiv = d.out_div, oslope = d.out_slope;
        for (int m = tid / BNV; m < BM; m += RSTEP) {
            const int po = out_off[m];
            if (po < 0) continue;
            const size_t o = (img + po) * d.Cout + co;
            const f32x4 v0 = *(const f32x4*)(ot + m * OS + vcol), v1 = *(const f32x4*)(ot + m * OS + vcol + 4);
            alignas(16) T mk[8], r1[8], r2[8], ov[8];
            if (ovec) {
                if (mask) *(u32x4*)mk = *(const u32x4*)(mask + o);
                if (res) *(u32x4*)r1 = *(const u32x4*)(res + o);
                if (res2) *(u32x4*)r2 = *(const u32x4*)(res2 + o);
            } else {
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const bool in = co + q < d.Cout;
                    if (mask) mk[q] = in ? mask[o + q] : (T)0;
                    if (res) r1[q] = in ? res[o + q] : (T)0;
                    if (res2) r2[q] = in ? res2[o + q] : (T)0;
                }
            }
            {                                                   // (cv_ep, conv.hip: one wave-uniform branch per optional operand)
                float xv[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) xv[q] = (q < 4 ? v0[q & 3] : v1[q & 3]) + bv[q];
                cv_ep<8>(xv, (const unsigned int*)mk, (const unsigned int*)r1, (const unsigned int*)r2, mask != nullptr,
                         res != nullptr, res2 != nullptr, mslope, odiv, oslope);
#pragma unroll
                for (int q = 0; q < 4; ++q) ((unsigned int*)ov)[q] = pack_bf16x2(xv[2 * q], xv[2 * q + 1]);
            }
            if (ovec) {
                *(u32x4*)(out + o) = *(const u32x4*)ov;
            } else {
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    if (co + q < d.Cout) out[o + q] = ov[q];
            }
        }
    }
}

template <int WM, int NTW, int CKM, int XV, bool XD>
__global__ __launch_bounds__(256) void conv_gather3_kernel(msmc_conv_desc d, CvGeom G) {
    cv3_body<WM, NTW, CKM, XV, XD>(d, G, blockIdx.x, blockIdx.y);
}
template <int WM, int NTW, int CKM, int XV, bool XD>
__global__ __launch_bounds__(256) void conv_gather3_group_kernel(CvGroupArgs a) {
    const int k = cv_group_member(a.first, a.n);
    const int id = blockIdx.x - a.first[k];
    cv3_body<WM, NTW, CKM, XV, XD>(a.d[k], a.G[k], id % a.nx[k], id / a.nx[k]);
}

// variant code of a third-generation configuration: 16 + (WM == 4) + 2 * (NTW == 2) + 4 * (CKM == 2); 16..23
// (+ 8: halo tile by LDS-DMA; 24..31)
static bool cv3_is_variant(int variant) { return variant >= 16 && variant < 32; }

static int cv3_plan(const msmc_conv_desc* d, int variant, Cv3Plan* pl) {
    pl->applies = 0;
    if (d->dtype != 1 || !cv3_is_variant(variant)) return 0;
    const int code = (variant - 16) & 7;
    const bool xdma = variant >= 24;
    // retired in round 6 (no decision of the tuned table over configurations 1-5, not instantiated any more): two column tiles
    // per wave WITH 64-channel chunks on the register-staged halo (22, 23) and its 128-point LDS-DMA form (30)
    if (variant == 22 || variant == 23 || variant == 30) return 0;
    const int wm = (code & 1) ? 4 : 2, ntw = (code & 2) ? 2 : 1, ckm = (code & 4) ? 2 : 1;
    const int wn = 4 / wm, bm = 64 * wm, bn = 32 * ntw * wn, ck = 32 * ckm, xs = ck + 8;
    if (d->Cin % ck != 0 || d->ntaps <= 0 || d->ntaps > MSMC_CONV_MAX_TAPS) return 0;
    if (xdma && !(d->in_slope >= 0.f && d->in_slope <= 1.f)) return 0;   // (the in-place pass computes max(x, slope * x))
    if ((long)d->Hin * d->Win * d->Cin >= (1L << 31) || (long)d->Hout * d->Wout >= (1L << 31)) return 0;
    if (((size_t)d->x | (size_t)d->w) & 15) return 0;
    if (bn >= 2 * d->Cout && bn > 32) return 0;                 // more than half of the tile would be padding
    size_t unused;
    int rc = cv_geometry(d, &pl->G, 2, xs, bn, &unused, bm);
    if (rc) return rc;
    const long npix = (long)pl->G.IH * pl->G.IW;
    const long xvec = npix * (ck / 8);
    const int xv = (int)((xvec + 255) / 256);
    if (xv > CV3_MAX_XV) return 0;
    const size_t tables = (((size_t)(npix + bm + 32) * sizeof(int)) + 15) & ~(size_t)15;
    const size_t xbytes = xdma ? ((((size_t)npix * ck * 2) + 1023) & ~(size_t)1023) : ((((size_t)npix * xs * 2) + 15) & ~(size_t)15);
    const size_t wbytes = (size_t)d->ntaps * bn * ck * 2;
    const size_t stage = 2 * xbytes + 2 * wbytes;
    const size_t epi = (size_t)bm * (bn + 4) * sizeof(float);
    const size_t lds = tables + (stage > epi ? stage : epi);
    if (lds > 160 * 1024) return 0;
    pl->applies = 1;
    pl->wm = wm; pl->ntw = ntw; pl->ckm = ckm;
    pl->xv = xdma ? 12 : xv <= 3 ? 3 : xv <= 6 ? 6 : 12;      // (the DMA form keeps one offset per piece: one instantiation)
    pl->xdma = xdma ? 1 : 0;
    pl->lds = lds;
    pl->gx = (unsigned)(pl->G.tilesX * pl->G.tilesY * d->B);
    pl->gy = (unsigned)((d->Cout + bn - 1) / bn);
    return 0;
}

#define CV3_INST(WM_, NTW_, CKM_, XV_, XD_)                                                                        \
    do {                                                                                                           \
        if (group) {                                                                                               \
            rc = msmc_allow_lds((const void*)conv_gather3_group_kernel<WM_, NTW_, CKM_, XV_, XD_>, (int)lds);      \
            if (rc) return rc;                                                                                     \
            MSMC_LAUNCH((conv_gather3_group_kernel<WM_, NTW_, CKM_, XV_, XD_>), grid, dim3(256), lds,              \
                        (msmc_stream_t)stream, *group);                                                            \
        } else {                                                                                                   \
            rc = msmc_allow_lds((const void*)conv_gather3_kernel<WM_, NTW_, CKM_, XV_, XD_>, (int)lds);            \
            if (rc) return rc;                                                                                     \
            MSMC_LAUNCH((conv_gather3_kernel<WM_, NTW_, CKM_, XV_, XD_>), grid, dim3(256), lds,                    \
                        (msmc_stream_t)stream, *d, *G);                                                            \
        }                                                                                                          \
    } while (0)
static int cv3_dispatch(const Cv3Plan& pl, dim3 grid, size_t lds, msmc_stream stream, const msmc_conv_desc* d,
                        const CvGeom* G, const CvGroupArgs* group) {
    int rc;
#define CV3_XV(WM_, NTW_, CKM_)                                                                                    \
    do {                                                                                                           \
        if (pl.xdma) CV3_INST(WM_, NTW_, CKM_, 12, true);                                                          \
        else if (pl.xv == 3) CV3_INST(WM_, NTW_, CKM_, 3, false);                                                  \
        else if (pl.xv == 6) CV3_INST(WM_, NTW_, CKM_, 6, false);                                                  \
        else CV3_INST(WM_, NTW_, CKM_, 12, false);                                                                 \
    } while (0)
#define CV3_CK(WM_, NTW_)                                                                                          \
    do {                                                                                                           \
        if (pl.ckm == 2) CV3_XV(WM_, NTW_, 2);                                                                     \
        else CV3_XV(WM_, NTW_, 1);                                                                                 \
    } while (0)
    // (NTW == 2 with 64-channel chunks exists as the LDS-DMA form of the 256-point tile only: variant 31)
    if (pl.wm == 2 && pl.ntw == 2) CV3_XV(2, 2, 1);
    else if (pl.wm == 2) CV3_CK(2, 1);
    else if (pl.ntw == 2) {
        if (pl.ckm == 2) CV3_INST(4, 2, 2, 12, true);
        else CV3_XV(4, 2, 1);
    } else CV3_CK(4, 1);
#undef CV3_CK
#undef CV3_XV
    static thread_local char name[96];
    snprintf(name, sizeof(name), "%s<%d, %d, %d, %d, %s>", group ? "conv_gather3_group_kernel" : "conv_gather3_kernel",
             pl.wm, pl.ntw, pl.ckm, pl.xv, pl.xdma ? "true" : "false");
    msmc_conv_last = msmc_prof_name(name);
    return msmc_check_launch();
}

// one descriptor on the third generation: 1 = launched, 0 = does not apply, < 0 error
static int cv3_launch(const msmc_conv_desc* d, msmc_stream stream) {
    Cv3Plan pl;
    int rc = cv3_plan(d, d->variant, &pl);
    if (rc) return rc;
    if (!pl.applies) return 0;
    rc = cv3_dispatch(pl, dim3(pl.gx, pl.gy), pl.lds, stream, d, &pl.G, nullptr);
    return cv_launched(rc);
}

// members of a grouped call (cv_family_group_launch): one grid per configuration (tile shape, chunk, halo registers)
struct Cv3Family {
    typedef Cv3Plan Plan;
    typedef CvGroupArgs Args;
    static constexpr int min_members = 1;
    static constexpr bool lone_single = true;
    static bool mine(const msmc_conv_desc* d) { return cv3_is_variant(d->variant); }
    static int plan(const msmc_conv_desc* d, Plan* pl, int) { return cv3_plan(d, d->variant, pl); }
    static bool same(const Plan& p, const Plan& q) {
        return p.wm == q.wm && p.ntw == q.ntw && p.ckm == q.ckm && p.xv == q.xv && p.xdma == q.xdma;
    }
    static int blocks(const Plan& p) { return (int)(p.gx * p.gy); }
    static int* head(Args& a, int m) { a.n = m; return a.first; }
    static void fill(Args& a, int k, const msmc_conv_desc& d, const Plan& p) {
        a.nx[k] = (int)p.gx;
        a.d[k] = d;
        a.G[k] = p.G;
    }
    static int dispatch(const Plan& p, int blocks, size_t lds, msmc_stream stream, const msmc_conv_desc* d, const Args* group) {
        return cv3_dispatch(p, group ? dim3((unsigned)blocks) : dim3(p.gx, p.gy), lds, stream, d, &p.G, group);
    }
};
