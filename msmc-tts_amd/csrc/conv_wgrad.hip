// conv_wgrad.hip -- weight gradients of the channels-last convolution family (conv.hip) for gfx950 (matrix cores).
//
// conv_wgrad_kernel<T>: dW[t][co][ci] += sum_{b,q} g[q][co] * act(x[in(q,t)][ci]); the reduction runs
//   over pixels, so both operands are transposed on their way into LDS (4x4 register transposes,
//   8-byte LDS writes) and every tap accumulates into its own fragment of the same wave.
#include <msmc_rt.hpp>
#include <msmc_hip.h>
#include <msmc_hip_debug.h>
#include "conv_common.inc"

static int msmc_wgrad_generation = 2;           // 1 = first-generation bf16 weight-gradient kernel (A/B tests)
extern "C" void msmc_conv_set_wgrad_generation(int n) { msmc_wgrad_generation = n; }
static int msmc_wgrad_tpw_cap = 5;              // accumulators per wave of the second-generation weight gradient (perf sweeps)
extern "C" void msmc_conv_set_wgrad_tpw(int n) { msmc_wgrad_tpw_cap = n < 1 ? 1 : n > 5 ? 5 : n; }
static int msmc_wgrad_split_override = 0;       // tests / perf sweeps: force the pixel-split factor
extern "C" void msmc_conv_set_wgrad_split(int n) { msmc_wgrad_split_override = n; }

// ================================================================================================
// weight gradient
// ================================================================================================
// dW[t][co][ci] += sum over lattice points p of g[p][co] * act(x[in(p,t)][ci]).  The reduction runs over
// pixels, so the MFMA K dimension is the pixel axis while LDS holds both operands in their natural
// channels-last layout ([pixel][channel], staged with the same halo-tile code as the forward kernel):
//   bf16: fragments come from ds_read_b64_tr_b16 (hardware transpose), every lane addressing the
//         pixel row it is responsible for -- a tap is again a pure row offset;
//   fp32: v_mfma_f32_32x32x2_f32 takes one element per lane, read straight from the tile.
// One workgroup owns a 64(co) x 64(ci) tile of every tap (4 waves x 32x32 fragments x TAPS accumulators)
// and walks a range of 128-point lattice tiles; partial sums meet in fp32 atomics.
#define WG_TM 128      // lattice points per tile (upper bound; smaller tiles when the halo would not fit LDS)

template <typename T>
MSMC_DEV void wg_stage_x(T* xt, int XS, const msmc_conv_desc& d, const CvGeom& G, const T* xb, int c0, int iyBase,
                         int ixBase, int tid) {
    constexpr int VEC = Elt<T>::VEC, CKV = 64 / VEC;
    const int npix = G.IH * G.IW;
    const bool vec_ok = (d.Cin % VEC) == 0;
    for (int e = tid; e < npix * CKV; e += 256) {
        const int pi = e / CKV, v = e - pi * CKV;
        const int ry = pi / G.IW, rx = pi - ry * G.IW;
        int iy = iyBase + ry, ix = ixBase + rx;
        bool inside = true;
        if (d.pad_mode == 1) {
            iy = reflect_index(iy, d.Hin);
            ix = reflect_index(ix, d.Win);
        } else {
            inside = (iy >= 0) && (iy < d.Hin) && (ix >= 0) && (ix < d.Win);
        }
        const int c = c0 + v * VEC;
        alignas(16) T vals[VEC];
#pragma unroll
        for (int q = 0; q < VEC; ++q) vals[q] = 0;
        if (inside && c < d.Cin) {
            const T* src = xb + ((size_t)iy * d.Win + ix) * d.Cin + c;
            if (vec_ok) {
                *(u32x4*)vals = *(const u32x4*)src;
            } else {
#pragma unroll
                for (int q = 0; q < VEC; ++q)
                    if (c + q < d.Cin) vals[q] = src[q];
            }
            if (d.in_slope != 1.f) {
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    float f = Elt<T>::ld(&vals[q]);
                    f = f > 0.f ? f : f * d.in_slope;
                    Elt<T>::st(&vals[q], f);
                }
            }
        }
        *(u32x4*)(xt + (size_t)pi * XS + v * VEC) = *(const u32x4*)vals;
    }
}

template <typename T>
MSMC_DEV void wg_stage_g(T* gt, int XS, const msmc_conv_desc& d, const CvGeom& G, const T* gb, int c0, int qy0, int qx0,
                         int tid, int TM) {
    constexpr int VEC = Elt<T>::VEC, CKV = 64 / VEC;
    const bool vec_ok = (d.Cout % VEC) == 0;
    for (int e = tid; e < TM * CKV; e += 256) {
        const int m = e / CKV, v = e - m * CKV;
        const int mty = m / G.TW, mtx = m - mty * G.TW;
        const int qy = qy0 + mty, qx = qx0 + mtx;
        const int c = c0 + v * VEC;
        alignas(16) T vals[VEC];
#pragma unroll
        for (int q = 0; q < VEC; ++q) vals[q] = 0;
        if (mty < G.TH && qy < d.QH && qx < d.QW && c < d.Cout) {
            const int oy = d.oy0 + qy * d.osy, ox = d.ox0 + qx * d.osx;
            const T* src = gb + ((size_t)oy * d.Wout + ox) * d.Cout + c;
            if (vec_ok) {
                *(u32x4*)vals = *(const u32x4*)src;
            } else {
#pragma unroll
                for (int q = 0; q < VEC; ++q)
                    if (c + q < d.Cout) vals[q] = src[q];
            }
            if (d.mask_slope != 1.f) {
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    float f = Elt<T>::ld(&vals[q]);
                    f = f > 0.f ? f : f * d.mask_slope;
                    Elt<T>::st(&vals[q], f);
                }
            }
        }
        *(u32x4*)(gt + (size_t)m * XS + v * VEC) = *(const u32x4*)vals;
    }
}

// One tap, one 128-point tile: acc += G^T . X_t   (per wave: 32 co x 32 ci)
MSMC_DEV f32x16 wg_tap(const float* gt, const float* xt, int XS, const int* rowtab, int tapoff, int acol, int bcol, int g,
                       f32x16 acc, int TM) {
    for (int s = 0; s < TM / 2; ++s) {
        const int m = 2 * s + g;
        acc = mfma_f32_32x32x2(gt[(size_t)m * XS + acol], xt[(size_t)(rowtab[m] + tapoff) * XS + bcol], acc);
    }
    return acc;
}
MSMC_DEV bf16x8 wg_frag(const unsigned short* tile, int XS, int row0, int row1, int col) {
    u16x4 lo = lds_read_tr16(tile + (size_t)row0 * XS + col);
    u16x4 hi = lds_read_tr16(tile + (size_t)row1 * XS + col);
    u16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
}

// staging slots per work-item of the FAST weight-gradient path: 64 channels are 8 (bf16) / 16 (fp32) 16-byte
// vectors per pixel, so the fp32 kernel needs twice the slots for the same tile
template <typename T, int TAPS> struct WgSlots {
    static constexpr int X = sizeof(T) == 2 ? (TAPS > 8 ? 6 : 12) : 12, G = sizeof(T) == 2 ? 4 : 8;
};

template <typename T, int TAPS, bool FAST>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(msmc_conv_desc d, const T* __restrict__ gptr,
                                                        float* __restrict__ dw, float* __restrict__ db, CvGeom G,
                                                        int tilesPerWg, int totalTiles, int TM) {
    MSMC_DYN_LDS(smem);
    constexpr int XS = 64 + Elt<T>::VEC;
    T* xt = (T*)smem;                                   // [IH*IW][XS]
    T* gt = xt + (size_t)G.IH * G.IW * XS;              // [TM][XS]
    int* rowtab = (int*)(gt + (size_t)TM * XS);         // [TM] X-tile pixel row of lattice point m
    const int nks = TM >> 4;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, i = lane & 31, g = lane >> 5;
    const int wm = w >> 1, wn = w & 1;
    const int co0 = blockIdx.y * 64, ci0 = blockIdx.z * 64;
    const bool wave_live = (co0 + 32 * wm < d.Cout) && (ci0 + 32 * wn < d.Cin);
    for (int m = tid; m < TM; m += 256) {
        int mty = m / G.TW, mtx = m - mty * G.TW;
        rowtab[m] = (mty < G.TH) ? (mty * d.isy) * G.IW + mtx * d.isx : 0;
    }
    f32x16 acc[TAPS];
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    __syncthreads();

    // bf16: lane L of each 16-lane group addresses row (L>>2) of its 4-row block, 4 channels from (L&3)*4
    const int L = lane & 15, half = (lane >> 4) & 1;
    int xrow[16], grow[16];
    if (sizeof(T) == 2) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = 16 * (r >> 1) + 8 * g + 4 * (r & 1) + (L >> 2);
            grow[r] = m < TM ? m : 0;
            xrow[r] = m < TM ? rowtab[m] : 0;
        }
    }
    const int acol_tr = 32 * wm + 16 * half + 4 * (L & 3), bcol_tr = 32 * wn + 16 * half + 4 * (L & 3);

    if (d.dw_copies > 1) {                              // privatised accumulators: copy (split index mod R)
        const int copy = blockIdx.x % d.dw_copies;
        dw += (size_t)copy * d.ntaps * d.Cout * d.Cin;
        if (db) db += (size_t)copy * d.Cout;
    }
    const bool do_bias = (db != nullptr) && (blockIdx.z == 0);
    float bias_acc = 0.f;
    const int t0 = blockIdx.x * tilesPerWg;
    int t1 = t0 + tilesPerWg;
    if (t1 > totalTiles) t1 = totalTiles;

    // FAST: every work-item owns fixed 16-byte staging slots (tile-relative coordinates computed once); the
    // loads of tile t+1 are issued before the MFMAs of tile t and written to LDS afterwards.
    constexpr int VEC = Elt<T>::VEC, CKV = 64 / VEC, WG_XLD = WgSlots<T, TAPS>::X, WG_GLD = WgSlots<T, TAPS>::G;
    int x_ry[WG_XLD], x_rx[WG_XLD], x_dst[WG_XLD], g_m[WG_GLD], g_dst[WG_GLD];
    u32x4 xreg[WG_XLD], greg[WG_GLD];
    if (FAST) {
        const int npix = G.IH * G.IW;
#pragma unroll
        for (int j = 0; j < WG_XLD; ++j) {
            const int e = tid + 256 * j;
            x_dst[j] = -1; x_ry[j] = x_rx[j] = 0;
            if (e < npix * CKV) {
                const int pi = e / CKV, v = e - pi * CKV;
                x_ry[j] = pi / G.IW;
                x_rx[j] = pi - x_ry[j] * G.IW;
                x_dst[j] = pi * XS + v * VEC;
            }
        }
#pragma unroll
        for (int j = 0; j < WG_GLD; ++j) {
            const int e = tid + 256 * j;
            g_dst[j] = -1; g_m[j] = 0;
            if (e < TM * CKV) {
                g_m[j] = e / CKV;
                g_dst[j] = g_m[j] * XS + (e - g_m[j] * CKV) * VEC;
            }
        }
    }
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    auto fetch = [&](int tile) {
        int bt = tile;
        const int tx_ = bt % G.tilesX;
        bt /= G.tilesX;
        const int ty_ = bt % G.tilesY;
        const int b = bt / G.tilesY;
        const int qy0 = ty_ * G.TH, qx0 = tx_ * G.TW;
        const int iyBase = qy0 * d.isy + d.iy0 + G.dyMin, ixBase = qx0 * d.isx + d.ix0 + G.dxMin;
        const T* xb = (const T*)d.x + (size_t)b * d.Hin * d.Win * d.Cin;
        const T* gb = gptr + (size_t)b * d.Hout * d.Wout * d.Cout;
#pragma unroll
        for (int j = 0; j < WG_XLD; ++j) {
            xreg[j] = zero4;
            if (x_dst[j] < 0) continue;
            int iy = iyBase + x_ry[j], ix = ixBase + x_rx[j];
            bool inside = true;
            if (d.pad_mode == 1) {
                iy = reflect_index(iy, d.Hin);
                ix = reflect_index(ix, d.Win);
            } else {
                inside = (iy >= 0) && (iy < d.Hin) && (ix >= 0) && (ix < d.Win);
            }
            const int c = ci0 + (x_dst[j] % XS);
            if (inside && c < d.Cin) xreg[j] = *(const u32x4*)(xb + ((size_t)iy * d.Win + ix) * d.Cin + c);
        }
#pragma unroll
        for (int j = 0; j < WG_GLD; ++j) {
            greg[j] = zero4;
            if (g_dst[j] < 0) continue;
            const int m = g_m[j];
            const int mty = m / G.TW, mtx = m - mty * G.TW;
            const int qy = qy0 + mty, qx = qx0 + mtx;
            const int c = co0 + (g_dst[j] % XS);
            if (mty < G.TH && qy < d.QH && qx < d.QW && c < d.Cout) {
                const int oy = d.oy0 + qy * d.osy, ox = d.ox0 + qx * d.osx;
                greg[j] = *(const u32x4*)(gb + ((size_t)oy * d.Wout + ox) * d.Cout + c);
            }
        }
    };
    auto act = [&](u32x4 v, float slope) {
        if (slope == 1.f) return v;
        alignas(16) T vals[VEC];
        *(u32x4*)vals = v;
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
            float f = Elt<T>::ld(&vals[q]);
            f = f > 0.f ? f : f * slope;
            Elt<T>::st(&vals[q], f);
        }
        return *(const u32x4*)vals;
    };
    auto commit = [&]() {
#pragma unroll
        for (int j = 0; j < WG_XLD; ++j)
            if (x_dst[j] >= 0) *(u32x4*)(xt + x_dst[j]) = act(xreg[j], d.in_slope);
#pragma unroll
        for (int j = 0; j < WG_GLD; ++j)
            if (g_dst[j] >= 0) *(u32x4*)(gt + g_dst[j]) = act(greg[j], d.mask_slope);
    };

    if (FAST && t0 < t1) fetch(t0);
    for (int tile = t0; tile < t1; ++tile) {
        __syncthreads();
        if (FAST) {
            commit();
        } else {
            int bt = tile;
            const int tx_ = bt % G.tilesX;
            bt /= G.tilesX;
            const int ty_ = bt % G.tilesY;
            const int b = bt / G.tilesY;
            const int qy0 = ty_ * G.TH, qx0 = tx_ * G.TW;
            const int iyBase = qy0 * d.isy + d.iy0 + G.dyMin, ixBase = qx0 * d.isx + d.ix0 + G.dxMin;
            wg_stage_x<T>(xt, XS, d, G, (const T*)d.x + (size_t)b * d.Hin * d.Win * d.Cin, ci0, iyBase, ixBase, tid);
            wg_stage_g<T>(gt, XS, d, G, gptr + (size_t)b * d.Hout * d.Wout * d.Cout, co0, qy0, qx0, tid, TM);
        }
        __syncthreads();
        if (FAST && tile + 1 < t1) fetch(tile + 1);
        if (do_bias && tid < 64) {                      // bias gradient: column sums of the g tile (fused)
            float sacc = 0.f;
            for (int m = 0; m < TM; ++m) sacc = sacc + Elt<T>::ld(gt + (size_t)m * XS + tid);
            bias_acc = bias_acc + sacc;
        }
        if (!wave_live) continue;
        if (sizeof(T) == 2) {
            // K-step outer, taps inner: one A fragment (g tile) live at a time, reused by every tap
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                if (ks >= nks) continue;
                const bf16x8 af = wg_frag((const unsigned short*)gt, XS, grow[2 * ks], grow[2 * ks + 1], acol_tr);
#pragma unroll
                for (int t = 0; t < TAPS; ++t) {
                    if (t < d.ntaps) {
                        const int tapoff = (d.tap_dy[t] - G.dyMin) * G.IW + (d.tap_dx[t] - G.dxMin);
                        const bf16x8 bf = wg_frag((const unsigned short*)xt, XS, xrow[2 * ks] + tapoff,
                                                  xrow[2 * ks + 1] + tapoff, bcol_tr);
                        acc[t] = mfma_bf16_32x32x16(af, bf, acc[t]);
                    }
                }
            }
        } else {
#pragma unroll
            for (int t = 0; t < TAPS; ++t) {
                if (t < d.ntaps) {
                    const int tapoff = (d.tap_dy[t] - G.dyMin) * G.IW + (d.tap_dx[t] - G.dxMin);
                    acc[t] = wg_tap((const float*)gt, (const float*)xt, XS, rowtab, tapoff, 32 * wm + i, 32 * wn + i, g,
                                    acc[t], TM);
                }
            }
        }
    }
    if (do_bias && tid < 64 && co0 + tid < d.Cout) atomicAdd(db + co0 + tid, bias_acc);
    // D fragment: row (co) = 32*wm + (r&3) + 8*(r>>2) + 4*g, col (ci) = 32*wn + i
    const int ci = ci0 + 32 * wn + i;
    if (!wave_live || ci >= d.Cin) return;
#pragma unroll
    for (int t = 0; t < TAPS; ++t) {
        if (t >= d.ntaps) continue;
        float* dst = dw + (size_t)d.tap_w[t] * d.Cout * d.Cin;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + 32 * wm + (r & 3) + 8 * (r >> 2) + 4 * g;
            if (co < d.Cout) atomicAdd(dst + (size_t)co * d.Cin + ci, acc[t][r]);
        }
    }
}

template <typename T>
static int wg_launch(const msmc_conv_desc* d, const void* g, float* dw, float* db, msmc_stream stream) {
    constexpr int XS = 64 + Elt<T>::VEC;
    CvGeom G;
    size_t lds_unused;
    int TM = WG_TM, rc;
    size_t lds;
    for (;;) {                                     // shrink the lattice tile until halo + g tile fit LDS
        rc = cv_geometry(d, &G, sizeof(T), XS, 0, &lds_unused, TM);
        if (rc) return rc;
        TM = ((G.TH * G.TW + 15) / 16) * 16;       // e.g. 11 x 11 MPD tile -> 128 rows, the tail rows are zero
        lds = ((size_t)G.IH * G.IW + TM) * XS * sizeof(T) + TM * sizeof(int);
        if (lds <= 160 * 1024) break;
        if (G.TH * G.TW <= 16) return MSMC_E_SHAPE;
        TM = (G.TH * G.TW) / 2;
    }
    const int totalTiles = G.tilesX * G.tilesY * d->B;
    const int ctiles = ((d->Cout + 63) / 64) * ((d->Cin + 63) / 64);
    // Split of the pixel reduction over workgroups: each split costs one fp32 atomic per dW element, and atomics
    // on ONE address retire serially at ~0.1 us each, so  t(n) = (tiles/n) * t_tile + n * 0.1 us  (t_tile ~3 us)
    // is minimal at n = sqrt(30 * tiles); never more workgroups than ~2 per CU.
    int nsplit = (int)(sqrt(30.0 * totalTiles * (d->dw_copies > 1 ? d->dw_copies : 1)) + 0.5);
    if (d->split_shift > 0) nsplit <<= d->split_shift;
    else if (d->split_shift < 0) nsplit >>= -d->split_shift;
    const int cap = (2 * MSMC_NUM_CU + ctiles - 1) / ctiles;
    if (msmc_wgrad_split_override > 0) nsplit = msmc_wgrad_split_override;
    else if (nsplit > cap) nsplit = cap;
    if (nsplit > totalTiles) nsplit = totalTiles;
    if (nsplit < 1) nsplit = 1;
    const int tilesPerWg = (totalTiles + nsplit - 1) / nsplit;
    nsplit = (totalTiles + tilesPerWg - 1) / tilesPerWg;
    dim3 grid((unsigned)nsplit, (unsigned)((d->Cout + 63) / 64), (unsigned)((d->Cin + 63) / 64));
    const T* gp = (const T*)g;
    constexpr int CKVh = 64 / Elt<T>::VEC;
    const int xslots = d->ntaps <= 4 ? WgSlots<T, 4>::X : d->ntaps <= 8 ? WgSlots<T, 8>::X : WgSlots<T, 12>::X;
    const bool fast = (d->Cin % Elt<T>::VEC) == 0 && (d->Cout % Elt<T>::VEC) == 0 && d->ntaps <= 12 &&
                      (long)G.IH * G.IW * CKVh <= 256L * xslots && (long)TM * CKVh <= 256L * WgSlots<T, 4>::G &&
                      msmc_conv_pipeline_enabled;
#define WG_GO(TP)                                                                                              \
    do {                                                                                                       \
        if (fast) {                                                                                            \
            rc = msmc_allow_lds((const void*)conv_wgrad_kernel<T, TP, true>, (int)lds);                        \
            if (rc) return rc;                                                                                 \
            MSMC_LAUNCH((conv_wgrad_kernel<T, TP, true>), grid, dim3(256), lds, (msmc_stream_t)stream, *d, gp, \
                        dw, db, G, tilesPerWg, totalTiles, TM);                                                \
        } else {                                                                                               \
            rc = msmc_allow_lds((const void*)conv_wgrad_kernel<T, TP, false>, (int)lds);                       \
            if (rc) return rc;                                                                                 \
            MSMC_LAUNCH((conv_wgrad_kernel<T, TP, false>), grid, dim3(256), lds, (msmc_stream_t)stream, *d, gp,\
                        dw, db, G, tilesPerWg, totalTiles, TM);                                                \
        }                                                                                                      \
    } while (0)
    if (d->ntaps <= 4) WG_GO(4);
    else if (d->ntaps <= 8) WG_GO(8);
    else if (d->ntaps <= 12) WG_GO(12);
    else WG_GO(16);
#undef WG_GO
    msmc_conv_last = msmc_prof_name(msmc_kname("conv_wgrad_kernel", EltName<T>::v,
                                               d->ntaps <= 4 ? 4 : d->ntaps <= 8 ? 8 : d->ntaps <= 12 ? 12 : 16, fast ? 1 : 0));
    return msmc_check_launch();
}


// ------------------------------------------------------------------------------------------------
// bf16 weight gradient, second generation.  Same math and LDS operand layout as conv_wgrad_kernel, but
//   * a wave owns one 32-channel block of output channels (its A fragment, read once per 16 pixels) and up
//     to TPW (input-channel block, tap) units of it -- with 32 or fewer channels the taps are spread over
//     all four waves instead of leaving three idle, and taps beyond the per-wave budget go to another
//     workgroup (grid.z), so no wave carries more than 5 accumulators and two or three workgroups fit a CU;
//   * staging vectors are as wide as the channel count allows (2..16 bytes), and the LDS rows hold only
//     the real channels: thin layers (2, 4, 8 channels) stage kilobytes, not 64-channel padded rows;
//   * the bias gradient is accumulated from the staged registers (no LDS pass);
//   * tile coordinates come from LDS tables built once per workgroup.
// ------------------------------------------------------------------------------------------------
struct Wg2Params {
    float* ws;               // third generation: per-split partial results [nsplit][ws_stride] (dW then db), NULL = none
    long ws_stride;          // floats per split region
    int direct;              // 1: this launch owns every dW element exactly once -> plain (non-atomic) accumulation
    int TM, tilesPerWg, totalTiles;
    int XSx, XSg;            // LDS row strides (elements)
    int vex, veg;            // elements per staging vector (1, 2, 4, 8)
    int shx, shg;            // log2(staging vectors per pixel)
    int TG, ntg;             // taps per workgroup, tap groups
};

template <int VE> struct WgVec;
template <> struct WgVec<8> { typedef u32x4 type; };
template <> struct WgVec<4> { typedef u32x2 type; };
template <> struct WgVec<2> { typedef unsigned int type; };
template <> struct WgVec<1> { typedef unsigned short type; };

template <int VE, bool SUM>
MSMC_DEV typename WgVec<VE>::type wg2_act(typename WgVec<VE>::type v, float slope, float (&sums)[8]) {
    typedef typename WgVec<VE>::type V;
    if (slope == 1.f && !SUM) return v;
    alignas(16) unsigned short vals[VE];
    *(V*)vals = v;
#pragma unroll
    for (int q = 0; q < VE; ++q) {
        float f = bf16_bits_to_f32(vals[q]);
        if (slope != 1.f) {
            f = f > 0.f ? f : f * slope;
            vals[q] = f32_to_bf16_bits(f);
        }
        if (SUM) sums[q] = sums[q] + f;
    }
    return *(const V*)vals;
}

// input halo tile -> LDS rows [pixel][channel]; padding rule and input activation applied here
template <int VE>
MSMC_DEV void wg2_stage_x(unsigned short* xt, const int* xmeta, const msmc_conv_desc& d, const unsigned short* xb,
                          int ci0, int iyBase, int ixBase, int npix, int sh, int XS, int tid) {
    typedef typename WgVec<VE>::type V;
    float unused[8];
    const int nvec = npix << sh, vmask = (1 << sh) - 1;
    for (int e0 = tid; e0 < nvec; e0 += 1024) {
        V vals[4];
        int dst[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + 256 * u;
            dst[u] = -1;
            vals[u] = V();
            if (e < nvec) {
                const int pi = e >> sh, c = (e & vmask) * VE;
                const int meta = xmeta[pi];
                int iy = iyBase + (meta >> 16), ix = ixBase + (meta & 0xffff);
                bool inside = true;
                if (d.pad_mode == 1) {
                    iy = reflect_index(iy, d.Hin);
                    ix = reflect_index(ix, d.Win);
                } else {
                    inside = (iy >= 0) && (iy < d.Hin) && (ix >= 0) && (ix < d.Win);
                }
                if (ci0 + c < d.Cin) {
                    dst[u] = pi * XS + c;
                    if (inside) vals[u] = *(const V*)(xb + ((size_t)iy * d.Win + ix) * d.Cin + ci0 + c);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (dst[u] >= 0) *(V*)(xt + dst[u]) = wg2_act<VE, false>(vals[u], d.in_slope, unused);
    }
}

// output-gradient tile -> LDS rows [lattice point][channel]; per-thread column sums feed the bias gradient
template <int VE, bool SUM>
MSMC_DEV void wg2_stage_g(unsigned short* gt, const int* gmeta, const msmc_conv_desc& d, const unsigned short* gb,
                          int co0, int qy0, int qx0, int TM, int sh, int XS, int tid, float (&sums)[8]) {
    typedef typename WgVec<VE>::type V;
    const int nvec = TM << sh, vmask = (1 << sh) - 1;
    for (int e0 = tid; e0 < nvec; e0 += 1024) {
        V vals[4];
        int dst[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + 256 * u;
            dst[u] = -1;
            vals[u] = V();
            if (e < nvec) {
                const int m = e >> sh, c = (e & vmask) * VE;
                const int meta = gmeta[m];
                if (co0 + c < d.Cout) {
                    dst[u] = m * XS + c;
                    const int qy = qy0 + (meta >> 16), qx = qx0 + (meta & 0xffff);
                    if (meta >= 0 && qy < d.QH && qx < d.QW) {
                        const int oy = d.oy0 + qy * d.osy, ox = d.ox0 + qx * d.osx;
                        vals[u] = *(const V*)(gb + ((size_t)oy * d.Wout + ox) * d.Cout + co0 + c);
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (dst[u] >= 0) *(V*)(gt + dst[u]) = wg2_act<VE, SUM>(vals[u], d.mask_slope, sums);
    }
}

template <int TPW>
MSMC_DEV void wg2_body(const msmc_conv_desc& d, const unsigned short* __restrict__ gptr, float* __restrict__ dw,
                       float* __restrict__ db, const CvGeom& G, const Wg2Params& P, const int block_x, const int block_y,
                       const int block_z) {
    MSMC_DYN_LDS(smem);
    const int npix = G.IH * G.IW, TM = P.TM, XSx = P.XSx, XSg = P.XSg;
    unsigned short* xt = (unsigned short*)smem;                  // [npix][XSx]
    unsigned short* gt = xt + (((size_t)npix * XSx + 7) & ~(size_t)7);   // [TM][XSg], 16-byte aligned
    int* xmeta = (int*)(gt + (size_t)TM * XSg);                  // [npix] (ry << 16) | rx
    int* gmeta = xmeta + npix;                                   // [TM]   (mty << 16) | mtx, -1 past the tile
    const int tid = threadIdx.x, w = wave_uniform(tid >> 6), lane = tid & 63, L = lane & 15, half = (lane >> 4) & 1;
    const int g = lane >> 5;
    const int co0 = block_y * 64;
    const int ciTile = block_z / P.ntg, tg = block_z - ciTile * P.ntg;
    const int ci0 = ciTile * 64;
    for (int pi = tid; pi < npix; pi += 256) {
        const int ry = pi / G.IW;
        xmeta[pi] = (ry << 16) | (pi - ry * G.IW);
    }
    for (int m = tid; m < TM; m += 256) {
        const int mty = m / G.TW;
        gmeta[m] = (mty < G.TH) ? ((mty << 16) | (m - mty * G.TW)) : -1;
    }
    __syncthreads();

    // ---- this wave's units: output-channel block cb, then (input-channel block, tap) pairs
    const int coLeft = d.Cout - co0, ciLeft = d.Cin - ci0;
    const int n_cb = coLeft > 32 ? 2 : 1, n_ib = ciLeft > 32 ? 2 : 1;
    const int wpc = 4 / n_cb, cb = w % n_cb, slot = w / n_cb;
    const int tap0 = tg * P.TG;
    int ntl = d.ntaps - tap0;
    if (ntl > P.TG) ntl = P.TG;
    const int nunits = n_ib * ntl;
    const int cpx = ((ciLeft > 64 ? 64 : ciLeft) + 3) & ~3, cpg = ((coLeft > 64 ? 64 : coLeft) + 3) & ~3;
    int boff[TPW], utap[TPW], uib[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        const int u = slot + wpc * j;
        utap[j] = -1; uib[j] = 0; boff[j] = 0;
        if (u < nunits) {
            const int ib = u % n_ib, t = tap0 + u / n_ib;
            int col = 32 * ib + 16 * half + 4 * (L & 3);
            if (col > cpx - 4) col = cpx - 4;           // thin tiles: surplus lanes re-read the last real chunk
            utap[j] = t; uib[j] = ib;
            boff[j] = ((d.tap_dy[t] - G.dyMin) * G.IW + (d.tap_dx[t] - G.dxMin)) * XSx + col;
        }
    }
    int acol = 32 * cb + 16 * half + 4 * (L & 3);
    if (acol > cpg - 4) acol = cpg - 4;
    // fragment rows: lane L of each 16-lane group addresses pixel row (L >> 2) of its 4-row block
    int xrow[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = 16 * (r >> 1) + 8 * g + 4 * (r & 1) + (L >> 2);
        int meta = m < TM ? gmeta[m] : -1;
        xrow[r] = meta >= 0 ? ((meta >> 16) * d.isy * G.IW + (meta & 0xffff) * d.isx) * XSx : 0;
    }
    f32x16 acc[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    const bool partial = P.ws != nullptr;               // plain stores into this split's workspace region
    if (partial) {
        dw = P.ws + (size_t)block_x * P.ws_stride;
        if (db) db = dw + (size_t)d.ntaps * d.Cout * d.Cin;
    } else if (d.dw_copies > 1 && !P.direct) {          // privatised accumulators: copy (split index mod R)
        const int copy = block_x % d.dw_copies;
        dw += (size_t)copy * d.ntaps * d.Cout * d.Cin;
        if (db) db += (size_t)copy * d.Cout;
    }
    const bool do_bias = (db != nullptr) && (block_z == 0);
    float bsum[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) bsum[q] = 0.f;
    const int nks = TM >> 4;
    const int t0 = block_x * P.tilesPerWg;
    int t1 = t0 + P.tilesPerWg;
    if (t1 > P.totalTiles) t1 = P.totalTiles;

    for (int tile = t0; tile < t1; ++tile) {
        int bt = tile;
        const int tx_ = bt % G.tilesX;
        bt /= G.tilesX;
        const int ty_ = bt % G.tilesY;
        const int b = bt / G.tilesY;
        const int qy0 = ty_ * G.TH, qx0 = tx_ * G.TW;
        const int iyBase = qy0 * d.isy + d.iy0 + G.dyMin, ixBase = qx0 * d.isx + d.ix0 + G.dxMin;
        const unsigned short* xb = (const unsigned short*)d.x + (size_t)b * d.Hin * d.Win * d.Cin;
        const unsigned short* gb = gptr + (size_t)b * d.Hout * d.Wout * d.Cout;
        __syncthreads();
        switch (P.vex) {
            case 8: wg2_stage_x<8>(xt, xmeta, d, xb, ci0, iyBase, ixBase, npix, P.shx, XSx, tid); break;
            case 4: wg2_stage_x<4>(xt, xmeta, d, xb, ci0, iyBase, ixBase, npix, P.shx, XSx, tid); break;
            case 2: wg2_stage_x<2>(xt, xmeta, d, xb, ci0, iyBase, ixBase, npix, P.shx, XSx, tid); break;
            default: wg2_stage_x<1>(xt, xmeta, d, xb, ci0, iyBase, ixBase, npix, P.shx, XSx, tid); break;
        }
#define WG2_STAGE_G(VE_)                                                                                      \
    do {                                                                                                      \
        if (do_bias) wg2_stage_g<VE_, true>(gt, gmeta, d, gb, co0, qy0, qx0, TM, P.shg, XSg, tid, bsum);      \
        else wg2_stage_g<VE_, false>(gt, gmeta, d, gb, co0, qy0, qx0, TM, P.shg, XSg, tid, bsum);             \
    } while (0)
        switch (P.veg) {
            case 8: WG2_STAGE_G(8); break;
            case 4: WG2_STAGE_G(4); break;
            case 2: WG2_STAGE_G(2); break;
            default: WG2_STAGE_G(1); break;
        }
#undef WG2_STAGE_G
        __syncthreads();
        if (utap[0] < 0) continue;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            if (ks >= nks) continue;
            const int m0 = 16 * ks + 8 * g + (L >> 2);
            const bf16x8 af = wg_frag(gt, 1, m0 * XSg, (m0 + 4) * XSg, acol);
#pragma unroll
            for (int j = 0; j < TPW; ++j) {
                if (utap[j] >= 0) {
                    const bf16x8 bf = wg_frag(xt, 1, xrow[2 * ks] + boff[j], xrow[2 * ks + 1] + boff[j], 0);
                    acc[j] = mfma_bf16_32x32x16(af, bf, acc[j]);
                }
            }
        }
    }

    if (do_bias) {
        // every work-item staged the same channel vector of each pixel it touched: combine the lanes that
        // share it, then the four waves through LDS -- ONE atomic per channel and workgroup (atomics on one
        // address retire at ~10 per microsecond on MI355X, whoever issues them)
        const int nv = 1 << P.shg, ve = P.veg;
        for (int mask = nv; mask < 64; mask <<= 1)
#pragma unroll
            for (int q = 0; q < 8; ++q) bsum[q] = bsum[q] + wave_xor(bsum[q], mask);
        float* red = (float*)smem;                      // [4][64]; the tiles are dead by now
        __syncthreads();
        if (lane < nv) {
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (q < ve) red[w * 64 + lane * ve + q] = bsum[q];
        }
        __syncthreads();
        if (tid < nv * ve && co0 + tid < d.Cout) {
            const float bs = ((red[tid] + red[64 + tid]) + red[128 + tid]) + red[192 + tid];
            if (partial) db[co0 + tid] = bs;
            else if (P.direct) db[co0 + tid] = db[co0 + tid] + bs;
            else atomicAdd(db + co0 + tid, bs);
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
            if (partial) *q = acc[j][r];
            else if (P.direct) *q = *q + acc[j][r];
            else atomicAdd(q, acc[j][r]);
        }
    }
}

// second stage of the third-generation weight gradient: the splits' partial results are summed in split order
// (bit-reproducible).  Small dW with many splits (thin layers over long signals) would leave this stage with a dozen
// workgroups, so it runs in two levels there: groups of consecutive splits are summed into `groups` intermediate
// regions (stored), then the groups are added to dW / db.  A member is one such pass: nsplit source regions of
// `stride` floats -> either an intermediate region (dst_ws) or the final dw | db pair.
template <int M>
struct WgReduceArgsT {
    int n;
    int first[M + 1];                       // first block of member k
    int eblocks[M];                         // blocks per group of member k (1024 floats each)
    const float* src[M];
    long stride[M];
    long n_dw[M];
    int nsplit[M], per_group[M], n_db[M];
    float* dst_ws[M];                       // not NULL: intermediate level, group gi stores its sums at dst_ws + gi * stride
    float* dw[M];                           // final level (one group): dw[e] += sum, db[e - n_dw] += sum
    float* db[M];
};
typedef WgReduceArgsT<MSMC_GROUP_MAX> WgReduceArgs;
// the merged second stage of a whole backward pass (msmc_conv_wgrad_reduce_pending): as many members per launch as a kernel
// argument block (4 KB) carries -- the discriminator's ~40 records went out as seven launches of six members, back to back on
// the critical chain in front of its optimizer step (profiles/r06_step_timeline_start_of_round.txt: 143 us)
#define WG_PENDING_MAX 40
typedef WgReduceArgsT<WG_PENDING_MAX> WgReduceArgsBig;
static_assert(sizeof(WgReduceArgsBig) <= 4000, "kernel argument block");
template <int M>
MSMC_DEV void wgrad_reduce_body(const WgReduceArgsT<M>& a) {
    int k = 0;
    while (k + 1 < a.n && (int)blockIdx.x >= a.first[k + 1]) ++k;
    const int id = blockIdx.x - a.first[k];
    const int gi = id / a.eblocks[k], eb = id - gi * a.eblocks[k];
    const long stride = a.stride[k], n_dw = a.n_dw[k], total = n_dw + a.n_db[k];
    const int s0 = gi * a.per_group[k];
    int S = a.nsplit[k] - s0;
    if (S > a.per_group[k]) S = a.per_group[k];
    const float* ws = a.src[k] + (size_t)s0 * stride;
    const long e0 = ((long)eb * 256 + threadIdx.x) * 4;
    if (e0 >= total || S <= 0) return;
    float* mid = a.dst_ws[k] ? a.dst_ws[k] + (size_t)gi * stride : nullptr;
    // (regions are padded to a multiple of four floats: an intermediate level may run past `total` inside them)
    if ((n_dw & 3) == 0 && (mid ? e0 + 4 <= stride : e0 + 4 <= n_dw)) {
        // (the splits are added in split order -- bit-reproducible -- but LOADED eight at a time: with one load in flight per
        //  work-item a member of 64 splits was 64 dependent memory round trips, and the pass ran at ~1 TB/s)
        // (round 6: a last batch of fewer than eight goes out together as well -- splits past the end re-read the last one and
        //  are not added; most members have 2-8 splits and ran entirely in the one-at-a-time remainder loop)
        f32x4 sum = *(const f32x4*)(ws + e0);
        for (int s_ = 1; s_ < S; s_ += 8) {
            f32x4 v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int sj = s_ + j < S ? s_ + j : S - 1;
                v[j] = *(const f32x4*)(ws + (size_t)sj * stride + e0);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (s_ + j < S) sum = sum + v[j];
        }
        if (mid) { *(f32x4*)(mid + e0) = sum; return; }
        f32x4* q = (f32x4*)(a.dw[k] + e0);
        *q = *q + sum;
        return;
    }
    for (long e = e0; e < e0 + 4 && e < total; ++e) {
        float sum = ws[e];
        for (int s_ = 1; s_ < S; ++s_) sum = sum + ws[(size_t)s_ * stride + e];
        if (mid) mid[e] = sum;
        else if (e < n_dw) a.dw[k][e] = a.dw[k][e] + sum;
        else if (a.db[k]) a.db[k][e - n_dw] = a.db[k][e - n_dw] + sum;
    }
}
__global__ __launch_bounds__(256) void conv_wgrad_reduce_kernel(WgReduceArgs a) { wgrad_reduce_body(a); }
__global__ __launch_bounds__(256) void conv_wgrad_reduce_pending_kernel(WgReduceArgsBig a) { wgrad_reduce_body(a); }

// plan of the second stage for one weight gradient: groups == 1 -> one level
struct Wg3Reduce {
    int groups, per_group;      // intermediate regions and splits per region (the last one may hold fewer)
};
static Wg3Reduce wg3_reduce_plan(long total, int nsplit) {
    Wg3Reduce r = {1, nsplit};
    const long echunks = (total + 1023) / 1024;
    if (nsplit >= 32 && echunks < 2 * MSMC_NUM_CU) {
        int groups = (int)((2 * MSMC_NUM_CU + echunks - 1) / echunks);
        if (groups > nsplit / 8) groups = nsplit / 8;
        if (groups > 32) groups = 32;
        if (groups > 1) {
            r.per_group = (nsplit + groups - 1) / groups;
            r.groups = (nsplit + r.per_group - 1) / r.per_group;
        }
    }
    return r;
}
// append the pass of one weight gradient at `level` (0: split groups -> intermediate regions, only when the plan has
// several groups; 1: -> dw | db) to a launch; `mid` = the intermediate regions (groups * stride floats)
// Deferred second stage (msmc_conv_wgrad_defer_begin / _end, include/msmc_hip.h): while the calling thread has a sink
// armed, the weight-gradient launchers record what their second stage would add up instead of launching it; the caller
// issues the recorded reductions of a whole backward pass together (msmc_conv_wgrad_reduce_pending).
static thread_local msmc_wg_pending* wg_defer_sink = nullptr;
static thread_local int wg_defer_cap = 0, wg_defer_n = 0;
template <int M>
static void wg3_reduce_add(WgReduceArgsT<M>& a, int* blocks, const float* ws, long stride, long n_dw, int n_db, int nsplit,
                           float* mid, float* dw, float* db, int level) {
    if (!ws) return;
    if (wg_defer_sink) {
        if (level == 0) {
            if (wg_defer_n < wg_defer_cap) {
                msmc_wg_pending& p = wg_defer_sink[wg_defer_n++];
                p.ws = ws; p.mid = mid; p.dw = dw; p.db = db;
                p.stride = stride; p.n_dw = n_dw; p.n_db = n_db; p.nsplit = nsplit;
                return;
            }
        } else {
            for (int i = 0; i < wg_defer_n; ++i)
                if (wg_defer_sink[i].ws == ws) return;      // recorded at level 0: nothing to launch now
        }
    }
    const long total = n_dw + n_db;
    const Wg3Reduce r = wg3_reduce_plan(total, nsplit);
    if (level == 0 && r.groups == 1) return;
    const int k = a.n++;
    a.first[k] = *blocks;
    a.eblocks[k] = (int)((total + 1023) / 1024);
    a.stride[k] = stride; a.n_dw[k] = n_dw; a.n_db[k] = n_db;
    if (level == 0) {
        a.src[k] = ws; a.nsplit[k] = nsplit; a.per_group[k] = r.per_group;
        a.dst_ws[k] = mid; a.dw[k] = nullptr; a.db[k] = nullptr;
        *blocks += a.eblocks[k] * r.groups;
    } else {
        a.src[k] = r.groups == 1 ? ws : mid;
        a.nsplit[k] = a.per_group[k] = r.groups == 1 ? nsplit : r.groups;
        a.dst_ws[k] = nullptr; a.dw[k] = dw; a.db[k] = db;
        *blocks += a.eblocks[k];
    }
}

template <int TPW>
__global__ __launch_bounds__(256, 2) void conv_wgrad2_kernel(msmc_conv_desc d, const unsigned short* __restrict__ gptr,
                                                            float* __restrict__ dw, float* __restrict__ db, CvGeom G,
                                                            Wg2Params P) {
    wg2_body<TPW>(d, gptr, dw, db, G, P, blockIdx.x, blockIdx.y, blockIdx.z);
}

// grouped weight gradients (see conv_gather2_group_kernel): members flattened over their (split, co tile, ci tile x taps)
struct Wg2GroupArgs {
    int n;
    int first[MSMC_GROUP_MAX + 1];
    int nx[MSMC_GROUP_MAX], ny[MSMC_GROUP_MAX];
    const unsigned short* g[MSMC_GROUP_MAX];
    float* dw[MSMC_GROUP_MAX];
    float* db[MSMC_GROUP_MAX];
    msmc_conv_desc d[MSMC_GROUP_MAX];
    CvGeom G[MSMC_GROUP_MAX];
    Wg2Params P[MSMC_GROUP_MAX];
};
template <int TPW>
__global__ __launch_bounds__(256, 2) void conv_wgrad2_group_kernel(Wg2GroupArgs a) {
    const int k = cv_group_member(a.first, a.n);
    int id = blockIdx.x - a.first[k];
    const int bx = id % a.nx[k];
    id /= a.nx[k];
    wg2_body<TPW>(a.d[k], a.g[k], a.dw[k], a.db[k], a.G[k], a.P[k], bx, id % a.ny[k], id / a.ny[k]);
}

static int wg2_vec_elems(int channels, const void* base) {
    int ve = 8;                                   // largest power of two dividing the pixel pitch and the base
    while (ve > 1 && ((channels % ve) != 0 || (((size_t)base) % (2 * ve)) != 0)) ve >>= 1;
    return ve;
}
static int wg2_row_stride(int cp) { return cp == 32 ? 48 : cp + 8; }   // rows of a 4-row transpose read on disjoint banks

struct Wg2Plan {
    Wg2Params P;
    CvGeom G;
    size_t lds;
    int tpw;
    unsigned gx, gy, gz;
    size_t ws_floats;            // third generation: workspace this launch needs (0: direct accumulation, one split)
};
#define WG3_WS_CAP_FLOATS (12L * 1024 * 1024)       // 48 MiB of partial results per launch at most
static int wg2_plan(const msmc_conv_desc* d, const void* g, Wg2Plan* pl, bool gen3 = false) {
    Wg2Params& P = pl->P;
    P.ws = nullptr;
    P.ws_stride = 0;
    P.direct = 0;
    pl->ws_floats = 0;
    const int cx = d->Cin > 64 ? 64 : d->Cin, cg = d->Cout > 64 ? 64 : d->Cout;
    P.vex = wg2_vec_elems(d->Cin, d->x);
    P.veg = wg2_vec_elems(d->Cout, g);
    P.shx = 0;
    while ((P.vex << P.shx) < cx) ++P.shx;
    P.shg = 0;
    while ((P.veg << P.shg) < cg) ++P.shg;
    P.XSx = wg2_row_stride((cx + 3) & ~3);
    P.XSg = wg2_row_stride((cg + 3) & ~3);
    CvGeom& G = pl->G;
    size_t lds_unused, lds;
    int TM = WG_TM, rc;
    for (;;) {                                     // shrink the lattice tile until two workgroups fit a CU
        rc = cv_geometry(d, &G, 2, P.XSx, 0, &lds_unused, TM);
        if (rc) return rc;
        TM = ((G.TH * G.TW + 15) / 16) * 16;
        lds = ((((size_t)G.IH * G.IW * P.XSx + 7) & ~(size_t)7) + (size_t)TM * P.XSg) * 2 +
              ((size_t)G.IH * G.IW + TM) * sizeof(int);
        if (lds <= 64 * 1024 && G.IH < 32768 && G.IW < 65536) break;
        if (G.TH * G.TW <= 16) {
            if (lds <= 160 * 1024) break;
            return MSMC_E_SHAPE;
        }
        TM = (G.TH * G.TW) / 2;
    }
    P.TM = TM;
    if (lds < 1024) lds = 1024;                  // the bias reduction reuses the first KiB
    // taps per workgroup: a wave carries at most 5 accumulators (6 would spill at two waves per SIMD)
    const int ncb = d->Cout > 32 ? 2 : 1, nib = d->Cin > 32 ? 2 : 1, wpc = 4 / ncb;
    int tgmax = msmc_wgrad_tpw_cap * wpc / nib;
    if (tgmax < 1) tgmax = 1;
    P.ntg = (d->ntaps + tgmax - 1) / tgmax;
    P.TG = (d->ntaps + P.ntg - 1) / P.ntg;
    const int tpw = (P.TG * nib + wpc - 1) / wpc;
    P.totalTiles = G.tilesX * G.tilesY * d->B;
    const int cols = ((d->Cout + 63) / 64) * ((d->Cin + 63) / 64) * P.ntg;
    // pixel split: every split adds one fp32 atomic per dW element, and atomics on ONE address retire serially at
    // ~0.1 us each (measured: 4096 per address -> 430 us), so  t(n) = (tiles/n) * t_tile + n * 0.1 us  with
    // t_tile ~3 us is minimal at n = sqrt(30 * tiles), whatever the size of dW
    int nsplit = (int)(sqrt(30.0 * P.totalTiles * (d->dw_copies > 1 ? d->dw_copies : 1)) + 0.5);
    if (d->split_shift > 0) nsplit <<= d->split_shift;
    else if (d->split_shift < 0) nsplit >>= -d->split_shift;
    const int cap = (4 * MSMC_NUM_CU + cols - 1) / cols;
    const long n_dw = (long)d->ntaps * d->Cout * d->Cin;
    const long stride = ((n_dw + d->Cout + 3) / 4) * 4;
    if (gen3) {
        // third generation: no atomics.  A split costs one plain store of its partial dW and one read in the second
        // stage, so the pixel reduction is split only as far as it takes to fill the chip (~3 workgroups per CU), and
        // never beyond the workspace cap; one split accumulates straight into dW.
        nsplit = (3 * MSMC_NUM_CU + cols - 1) / cols;
        if (d->split_shift > 0) nsplit <<= d->split_shift;
        else if (d->split_shift < 0) nsplit >>= -d->split_shift;
        const long fit = WG3_WS_CAP_FLOATS / stride;            // (the intermediate regions of a two-level second stage
        if (nsplit > fit) nsplit = (int)(fit > 1 ? fit : 1);    //  are at most an eighth on top)
    }
    if (msmc_wgrad_split_override > 0) nsplit = msmc_wgrad_split_override;
    else if (!gen3 && nsplit > cap) nsplit = cap;
    if (nsplit > P.totalTiles) nsplit = P.totalTiles;
    if (nsplit < 1) nsplit = 1;
    P.tilesPerWg = (P.totalTiles + nsplit - 1) / nsplit;
    nsplit = (P.totalTiles + P.tilesPerWg - 1) / P.tilesPerWg;
    if (gen3) {
        P.direct = nsplit == 1;
        P.ws_stride = stride;
        pl->ws_floats = nsplit > 1 ? (size_t)(nsplit + wg3_reduce_plan(n_dw + d->Cout, nsplit).groups) * stride : 0;
    }
    pl->lds = lds;
    pl->tpw = tpw <= 4 ? (tpw < 1 ? 1 : tpw) : 5;
    pl->gx = (unsigned)nsplit;
    pl->gy = (unsigned)((d->Cout + 63) / 64);
    pl->gz = (unsigned)(((d->Cin + 63) / 64) * P.ntg);
    return 0;
}

static int wg3_reduce_launch(WgReduceArgs& a, int blocks, msmc_stream stream) {
    MSMC_LAUNCH(conv_wgrad_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, (msmc_stream_t)stream, a);
    ++msmc_conv_launches;
    return msmc_check_launch();
}
// a single-descriptor launcher whose plan splits the pixels takes its `need` floats of partial results from the caller's workspace
static int wg3_take_ws(size_t need, float* ws, size_t ws_floats, float** slot) {
    if (!need) return 0;
    if (!ws || ws_floats < need) return MSMC_E_WORKSPACE;
    *slot = ws;
    return 0;
}
// second stage of a single-descriptor launcher: the nsplit partial results in ws (`stride` floats each) -> dw | db, in two
// levels where wg3_reduce_plan asks for them (the intermediate regions follow the partial results)
static int wg3_reduce_single(const msmc_conv_desc* d, float* ws, long stride, int nsplit, float* dw, float* db,
                             msmc_stream stream) {
    const long n_dw = (long)d->ntaps * d->Cout * d->Cin;
    float* mid = ws + (size_t)nsplit * stride;
    for (int level = 0; level < 2; ++level) {
        WgReduceArgs a;
        a.n = 0;
        int blocks = 0;
        wg3_reduce_add(a, &blocks, ws, stride, n_dw, db ? d->Cout : 0, nsplit, mid, dw, db, level);
        if (!a.n) continue;
        a.first[a.n] = blocks;
        int rc = wg3_reduce_launch(a, blocks, stream);
        if (rc) return rc;
    }
    return 0;
}

extern "C" void msmc_conv_wgrad_defer_begin(msmc_wg_pending* sink, int capacity) {
    wg_defer_sink = capacity > 0 ? sink : nullptr;
    wg_defer_cap = capacity;
    wg_defer_n = 0;
}
extern "C" int msmc_conv_wgrad_defer_end(void) {
    const int n = wg_defer_n;
    wg_defer_sink = nullptr;
    wg_defer_cap = wg_defer_n = 0;
    return n;
}
extern "C" int msmc_conv_wgrad_reduce_pending(const msmc_wg_pending* items, int n, msmc_stream stream) {
    if (n < 0 || (n && !items)) return MSMC_E_SHAPE;
    msmc_wg_pending* keep = wg_defer_sink;                  // (the merged launches themselves are never deferred)
    wg_defer_sink = nullptr;
    int rc = 0;
    for (int level = 0; level < 2 && !rc; ++level) {
        int i = 0;
        while (i < n && !rc) {
            WgReduceArgsBig a;
            a.n = 0;
            int blocks = 0;
            for (; i < n && a.n < WG_PENDING_MAX; ++i) {
                const msmc_wg_pending& p = items[i];
                if (level == 1) {
                    // a layer applied twice in one backward pass (D(real) and D(fake) as separate calls, rb(rb(x))) has two
                    // records with the same accumulator: their `dw += sum` are plain read-modify-writes, so they must not
                    // share a launch -- close this one, the next is ordered after it on the stream
                    bool clash = false;
                    for (int j = 0; j < a.n && !clash; ++j)
                        clash = (a.dw[j] && a.dw[j] == p.dw) || (a.db[j] && a.db[j] == p.db);
                    if (clash) break;
                }
                wg3_reduce_add(a, &blocks, p.ws, p.stride, p.n_dw, p.n_db, p.nsplit, p.mid, p.dw, p.db, level);
            }
            if (!a.n) continue;
            a.first[a.n] = blocks;
            MSMC_LAUNCH(conv_wgrad_reduce_pending_kernel, dim3((unsigned)blocks), dim3(256), 0, (msmc_stream_t)stream, a);
            ++msmc_conv_launches;
            rc = msmc_check_launch();
        }
    }
    wg_defer_sink = keep;
    return rc;
}

static int wg2_launch(const msmc_conv_desc* d, const void* g, float* dw, float* db, msmc_stream stream,
                      float* ws = nullptr, size_t ws_floats = 0) {
    Wg2Plan pl;
    const bool gen3 = d->variant == 3;
    int rc = wg2_plan(d, g, &pl, gen3);
    if (rc) return rc;
    if (gen3) rc = wg3_take_ws(pl.ws_floats, ws, ws_floats, &pl.P.ws);
    if (rc) return rc;
    const dim3 grid(pl.gx, pl.gy, pl.gz);
    const size_t lds = pl.lds;
    const unsigned short* gp = (const unsigned short*)g;
#define WG2_GO(TP)                                                                                           \
    do {                                                                                                     \
        rc = msmc_allow_lds((const void*)conv_wgrad2_kernel<TP>, (int)lds);                                  \
        if (rc) return rc;                                                                                   \
        MSMC_LAUNCH((conv_wgrad2_kernel<TP>), grid, dim3(256), lds, (msmc_stream_t)stream, *d, gp, dw, db, pl.G, pl.P); \
    } while (0)
    if (pl.tpw == 1) WG2_GO(1);
    else if (pl.tpw == 2) WG2_GO(2);
    else if (pl.tpw == 3) WG2_GO(3);
    else if (pl.tpw == 4) WG2_GO(4);
    else WG2_GO(5);
#undef WG2_GO
    msmc_conv_last = msmc_prof_name(msmc_kname("conv_wgrad2_kernel", nullptr, pl.tpw, -1));
    rc = msmc_check_launch();
    if (rc || !pl.P.ws) return rc;
    return wg3_reduce_single(d, ws, pl.P.ws_stride, (int)pl.gx, dw, db, stream);
}

#include "wgrad4.inc"

// fourth generation (variants 4 / 5 / 6, see wg4_plan): MSMC_E_SHAPE where it does not apply
static int wg4_launch(const msmc_conv_desc* d, const void* g, float* dw, float* db, msmc_stream stream, float* ws,
                      size_t ws_floats) {
    Wg4Plan pl;
    int rc = wg4_plan(d, g, &pl, d->variant - 4);
    if (rc) return rc;
    rc = wg3_take_ws(pl.ws_floats, ws, ws_floats, &pl.P.ws);
    if (rc) return rc;
    const dim3 grid(pl.gx, pl.gy, pl.gz);
    const unsigned short* gp = (const unsigned short*)g;
#define WG4_GO(TP, DD)                                                                                       \
    do {                                                                                                     \
        rc = msmc_allow_lds((const void*)conv_wgrad4_kernel<TP, DD>, (int)pl.lds);                           \
        if (rc) return rc;                                                                                   \
        MSMC_LAUNCH((conv_wgrad4_kernel<TP, DD>), grid, dim3(256), pl.lds, (msmc_stream_t)stream, *d, gp, dw, db, pl.P); \
    } while (0)
    const bool ahead2 = d->variant == 4;
    if (pl.tpw == 1) { if (ahead2) WG4_GO(1, 2); else WG4_GO(1, 1); }
    else if (pl.tpw == 2) { if (ahead2) WG4_GO(2, 2); else WG4_GO(2, 1); }
    else if (pl.tpw == 3) { if (ahead2) WG4_GO(3, 2); else WG4_GO(3, 1); }
    else if (pl.tpw == 4) { if (ahead2) WG4_GO(4, 2); else WG4_GO(4, 1); }
    else WG4_GO(5, 1);
#undef WG4_GO
    msmc_conv_last = msmc_prof_name(msmc_kname("conv_wgrad4_kernel", nullptr, pl.tpw, (ahead2 && pl.tpw < 5) ? 2 : 1));
    rc = msmc_check_launch();
    if (rc || !pl.P.ws) return rc;
    return wg3_reduce_single(d, ws, pl.P.ws_stride, (int)pl.gx, dw, db, stream);
}

#include "wgrad5.inc"
#include "wgrad6.inc"
#include "wgrad7.inc"

// general-lattice weight gradient with LDS-DMA staging (variant 7: interpreter-tested, not yet timed on the GPU)
static int wg5_launch(const msmc_conv_desc* d, const void* g, float* dw, float* db, msmc_stream stream, float* ws,
                      size_t ws_floats) {
    Wg5Plan pl;
    int rc = wg5_plan(d, g, &pl);
    if (rc) return rc;
    rc = wg3_take_ws(pl.ws_floats, ws, ws_floats, &pl.P.ws);
    if (rc) return rc;
    const dim3 grid(pl.gx, pl.gy, pl.gz);
    const unsigned short* gp = (const unsigned short*)g;
#define WG5_GO(TP)                                                                                           \
    do {                                                                                                     \
        rc = msmc_allow_lds((const void*)conv_wgrad5_kernel<TP>, (int)pl.lds);                               \
        if (rc) return rc;                                                                                   \
        MSMC_LAUNCH((conv_wgrad5_kernel<TP>), grid, dim3(256), pl.lds, (msmc_stream_t)stream, *d, gp, dw, db, pl.G, pl.P); \
    } while (0)
    if (pl.tpw == 1) WG5_GO(1);
    else if (pl.tpw == 2) WG5_GO(2);
    else if (pl.tpw == 3) WG5_GO(3);
    else if (pl.tpw == 4) WG5_GO(4);
    else WG5_GO(5);
#undef WG5_GO
    msmc_conv_last = msmc_prof_name(msmc_kname("conv_wgrad5_kernel", nullptr, pl.tpw, -1));
    rc = msmc_check_launch();
    if (rc || !pl.P.ws) return rc;
    return wg3_reduce_single(d, ws, pl.P.ws_stride, (int)pl.gx, dw, db, stream);
}

extern "C" int msmc_conv_wgrad_ws(const msmc_conv_desc* d, const void* g, float* dw, float* db, void* workspace,
                                  size_t workspace_bytes, msmc_stream stream) {
    if (!d || !g || !dw || !cv_desc_ok(d)) return MSMC_E_SHAPE;
    if (d->ntaps <= 0 || d->ntaps > MSMC_CONV_MAX_TAPS) return MSMC_E_SHAPE;
    ++msmc_conv_launches;
    if (d->dtype == 0) return d->variant == 3 ? MSMC_E_SHAPE : wg_launch<float>(d, g, dw, db, stream);
    if (d->dtype == 1) {
        const int gen = d->variant > 0 ? d->variant : msmc_wgrad_generation;
        if (gen == 1) return wg_launch<unsigned short>(d, g, dw, db, stream);
        msmc_conv_desc e = *d;
        e.variant = gen;                                      // (the generation switch selects the third one too)
        if (gen == 7) return wg5_launch(&e, g, dw, db, stream, (float*)workspace, workspace_bytes / sizeof(float));
        if (gen == 8) return wg6_launch(&e, g, dw, db, stream);      // direct thin-layer kernel (E_SHAPE outside its scope)
        if (gen == 9) return wg7_launch(&e, g, dw, db, stream, (float*)workspace, workspace_bytes / sizeof(float));   // 128 x 128 channel tiles
        if (gen >= 4) {
            if (gen > 6) return MSMC_E_SHAPE;
            const int rc = wg4_launch(&e, g, dw, db, stream, (float*)workspace, workspace_bytes / sizeof(float));
            if (rc != MSMC_E_SHAPE || d->variant > 0) return rc;
            e.variant = 3;                                    // forced through the global switch: third generation elsewhere
        }
        return wg2_launch(&e, g, dw, db, stream, (float*)workspace, workspace_bytes / sizeof(float));
    }
    return MSMC_E_SHAPE;
}
extern "C" int msmc_conv_wgrad(const msmc_conv_desc* d, const void* g, float* dw, float* db, msmc_stream stream) {
    return msmc_conv_wgrad_ws(d, g, dw, db, nullptr, 0, stream);
}
extern "C" size_t msmc_conv_wgrad_workspace(const msmc_conv_desc* d, const void* g) {
    if (!d || d->dtype != 1) return 0;
    const int gen = d->variant > 0 ? d->variant : msmc_wgrad_generation;
    size_t need4 = 0;
    if (gen == 7) {
        Wg5Plan p5;
        return wg5_plan(d, g, &p5) == 0 ? p5.ws_floats * sizeof(float) : 0;
    }
    if (gen == 9) {
        Wg4Plan p7;
        return wg7_plan(d, g, &p7) == 0 ? p7.ws_floats * sizeof(float) : 0;
    }
    if (gen >= 4 && gen <= 6) {                     // (inside a shared grid the member runs as third generation: the larger)
        Wg4Plan p4;
        if (wg4_plan(d, g, &p4, gen - 4) == 0) need4 = p4.ws_floats * sizeof(float);
    } else if (gen != 3) {
        return 0;
    }
    Wg2Plan pl;
    if (wg2_plan(d, g, &pl, true)) return need4;
    const size_t need3 = pl.ws_floats * sizeof(float);
    return need3 > need4 ? need3 : need4;
}

// ------------------------------------------------------------------------------------------------
// Grouped weight gradients of ONE kernel family.  A family is a traits struct F:
//   F::Plan, F::Args        plan of one member (P, lds, tpw, gx, gy, gz, ws_floats) / argument block of the group kernel
//   F::kernel<TPW>          the group kernel for TPW accumulators per wave; F::name, F::name_arg: its symbol as msmc_kname prints it
//   F::geom(a, k, p)        stores the member's lattice geometry where the argument block carries one
// and, for the families that select their own members (wg_family_group_launch):
//   F::owns(gen)            generations the family takes
//   F::plan(d, g, pl, gen, share)
// ------------------------------------------------------------------------------------------------
// the members todo[] (planned, workspace assigned) as launches of at most MSMC_GROUP_MAX members in member order: fill the
// argument block, launch the kernel of the widest member, then the two-level second stage of the members that split
template <class F>
static int wg_group_run(const msmc_conv_desc* descs, const void* const* g, float* const* dw, float* const* db, int n,
                        const typename F::Plan* pl, bool* todo, msmc_stream stream) {
    for (int i = 0; i < n; ++i) {
        if (!todo[i]) continue;
        typename F::Args a;
        a.n = 0;
        int members[MSMC_GROUP_MAX], nmembers = 0;            // members of this launch with a second stage
        int blocks = 0, tpw = 1;
        size_t lds = 0;
        for (int j = i; j < n && a.n < MSMC_GROUP_MAX; ++j) {
            if (!todo[j]) continue;
            const int k = a.n++;
            a.first[k] = blocks;
            a.nx[k] = (int)pl[j].gx;
            a.ny[k] = (int)pl[j].gy;
            a.g[k] = (const unsigned short*)g[j];
            a.dw[k] = dw[j];
            a.db[k] = db ? db[j] : nullptr;
            a.d[k] = descs[j];
            F::geom(a, k, pl[j]);
            a.P[k] = pl[j].P;
            blocks += (int)(pl[j].gx * pl[j].gy * pl[j].gz);
            if (pl[j].lds > lds) lds = pl[j].lds;
            if (pl[j].tpw > tpw) tpw = pl[j].tpw;              // the widest member sets the accumulator budget
            if (pl[j].P.ws) members[nmembers++] = j;
            todo[j] = false;
        }
        a.first[a.n] = blocks;
        ++msmc_conv_launches;
        int rc;
        const dim3 grid((unsigned)blocks);
#define WGG_GO(TP)                                                                                           \
    do {                                                                                                     \
        rc = msmc_allow_lds((const void*)F::template kernel<TP>, (int)lds);                                  \
        if (rc) return rc;                                                                                   \
        MSMC_LAUNCH((F::template kernel<TP>), grid, dim3(256), lds, (msmc_stream_t)stream, a);               \
    } while (0)
        if (tpw == 1) WGG_GO(1);
        else if (tpw == 2) WGG_GO(2);
        else if (tpw == 3) WGG_GO(3);
        else if (tpw == 4) WGG_GO(4);
        else WGG_GO(5);
#undef WGG_GO
        msmc_conv_last = msmc_prof_name(msmc_kname(F::name, nullptr, tpw, F::name_arg));
        rc = msmc_check_launch();
        if (rc) return rc;
        for (int level = 0; level < 2 && nmembers; ++level) {
            WgReduceArgs r;
            r.n = 0;
            int rblocks = 0;
            for (int q = 0; q < nmembers; ++q) {
                const int j = members[q];
                const msmc_conv_desc& dj = descs[j];
                float* wsj = pl[j].P.ws;
                wg3_reduce_add(r, &rblocks, wsj, pl[j].P.ws_stride, (long)dj.ntaps * dj.Cout * dj.Cin,
                               (db && db[j]) ? dj.Cout : 0, (int)pl[j].gx, wsj + (size_t)pl[j].gx * pl[j].P.ws_stride, dw[j],
                               db ? db[j] : nullptr, level);
            }
            if (!r.n) continue;
            r.first[r.n] = rblocks;
            rc = wg3_reduce_launch(r, rblocks, stream);
            if (rc) return rc;
        }
    }
    return 0;
}
// the family's members among those no family has taken yet: when there are several, each is planned for its share of the
// chip, takes the next region of the workspace and joins the family's grids.  A member whose plan fails stays with the
// paths after this one.
template <class F>
static int wg_family_group_launch(const msmc_conv_desc* descs, const void* const* g, float* const* dw, float* const* db, int n,
                                  bool* took, float** wsp, size_t* ws_left, msmc_stream stream) {
    typename F::Plan pl[MSMC_GROUP_LIMIT];
    bool mine[MSMC_GROUP_LIMIT];
    int left = 0, count = 0;
    for (int i = 0; i < n; ++i) {
        const msmc_conv_desc* d = &descs[i];
        const int gen = d->variant > 0 ? d->variant : msmc_wgrad_generation;
        mine[i] = !took[i] && d->dtype == 1 && F::owns(gen) && g[i] && dw[i] && d->B > 0 && d->ntaps > 0 &&
                  d->ntaps <= MSMC_CONV_MAX_TAPS;
        left += !took[i];
        count += mine[i];
    }
    if (left <= 1 || count <= 1) return 0;
    const int share = count < MSMC_GROUP_MAX ? count : MSMC_GROUP_MAX;
    for (int i = 0; i < n; ++i) {
        if (!mine[i]) continue;
        const msmc_conv_desc* d = &descs[i];
        if (F::plan(d, g[i], &pl[i], d->variant > 0 ? d->variant : msmc_wgrad_generation, share)) { mine[i] = false; continue; }
        if (pl[i].ws_floats) {
            if (pl[i].ws_floats > *ws_left) return MSMC_E_WORKSPACE;
            pl[i].P.ws = *wsp;
            *wsp += pl[i].ws_floats;
            *ws_left -= pl[i].ws_floats;
        }
        took[i] = true;
    }
    return wg_group_run<F>(descs, g, dw, db, n, pl, mine, stream);
}
struct Wg5Group {                   // general-lattice LDS-DMA members (variant 7)
    typedef Wg5Plan Plan;
    typedef Wg5GroupArgs Args;
    template <int TPW> static constexpr auto kernel = conv_wgrad5_group_kernel<TPW>;
    static constexpr const char* name = "conv_wgrad5_group_kernel";
    static constexpr int name_arg = -1;
    static void geom(Args& a, int k, const Plan& p) { a.G[k] = p.G; }
    static bool owns(int gen) { return gen == 7; }
    static int plan(const msmc_conv_desc* d, const void* g, Plan* pl, int, int share) { return wg5_plan(d, g, pl, share); }
};
struct Wg4Group {                   // fourth generation (variants 4 / 5 / 6 inside wgrad4.inc's scope)
    typedef Wg4Plan Plan;
    typedef Wg4GroupArgs Args;
    template <int TPW> static constexpr auto kernel = conv_wgrad4_group_kernel<TPW, 1>;
    static constexpr const char* name = "conv_wgrad4_group_kernel";
    static constexpr int name_arg = 1;
    static void geom(Args&, int, const Plan&) {}
    static bool owns(int gen) { return gen >= 4 && gen <= 6; }
    static int plan(const msmc_conv_desc* d, const void* g, Plan* pl, int gen, int share) { return wg4_plan(d, g, pl, gen - 4, share); }
};
struct Wg2Group {                   // second / third generation: msmc_conv_wgrad_group_ws4 selects and plans the members
    typedef Wg2Plan Plan;
    typedef Wg2GroupArgs Args;
    template <int TPW> static constexpr auto kernel = conv_wgrad2_group_kernel<TPW>;
    static constexpr const char* name = "conv_wgrad2_group_kernel";
    static constexpr int name_arg = -1;
    static void geom(Args& a, int k, const Plan& p) { a.G[k] = p.G; }
};

// n independent weight gradients (msmc_conv_wgrad semantics each): bf16 second- / third-generation members share grids.
// Third-generation members (variant 3) take consecutive regions of the workspace; one grouped second-stage launch
// folds the partial results of all of them.
// group4 != 0: variant-7 members, then fourth-generation members (variants 4 / 5 / 6 inside wgrad4.inc's scope) share grids of
// their own kernels (every member planned for its share of the chip); what they leave goes on as a call of its own would
// (one member left: a single launch).  0: fourth-generation members join the shared grid of the second / third generation
// as third-generation members.  The host layer times both against one launch per member.
extern "C" int msmc_conv_wgrad_group_ws4(const msmc_conv_desc* descs, const void* const* g, float* const* dw,
                                         float* const* db, int n, void* workspace, size_t workspace_bytes,
                                         msmc_stream stream, int group4) {
    if (!descs || !g || !dw || n <= 0 || n > MSMC_GROUP_LIMIT) return MSMC_E_SHAPE;
    Wg2Plan plans[MSMC_GROUP_LIMIT];
    bool pending[MSMC_GROUP_LIMIT], took[MSMC_GROUP_LIMIT] = {};
    float* wsp = (float*)workspace;
    size_t ws_left = workspace_bytes / sizeof(float);
    if (group4 && msmc_conv_grouping) {
        int rc = wg_family_group_launch<Wg5Group>(descs, g, dw, db, n, took, &wsp, &ws_left, stream);
        if (!rc) rc = wg_family_group_launch<Wg4Group>(descs, g, dw, db, n, took, &wsp, &ws_left, stream);
        if (rc) return rc;
    }
    int left = 0;
    for (int i = 0; i < n; ++i) left += !took[i];
    for (int i = 0; i < n; ++i) {
        const msmc_conv_desc* d = &descs[i];
        pending[i] = false;
        if (took[i]) continue;
        const int gen = d->variant > 0 ? d->variant : msmc_wgrad_generation;
        // (fourth-generation members join a shared grid as third-generation members: the host layer times the shared
        //  grid against one launch per member, where each runs the kernel of its own choice)
        if (!msmc_conv_grouping || d->dtype != 1 || gen == 1 || gen == 7 || gen == 8 || gen == 9 || left == 1) {
            size_t need = msmc_conv_wgrad_workspace(d, g[i]) / sizeof(float);
            if (need > ws_left) return MSMC_E_WORKSPACE;
            int rc = msmc_conv_wgrad_ws(d, g[i], dw[i], db ? db[i] : nullptr, wsp, need * sizeof(float), stream);
            if (rc) return rc;
            wsp += need;
            ws_left -= need;
            continue;
        }
        if (!g[i] || !dw[i] || !cv_desc_ok(d) || d->ntaps <= 0 || d->ntaps > MSMC_CONV_MAX_TAPS) return MSMC_E_SHAPE;
        int rc = wg2_plan(d, g[i], &plans[i], gen >= 3);
        if (rc) return rc;
        if (plans[i].ws_floats) {
            if (plans[i].ws_floats > ws_left) return MSMC_E_WORKSPACE;
            plans[i].P.ws = wsp;
            wsp += plans[i].ws_floats;
            ws_left -= plans[i].ws_floats;
        }
        pending[i] = true;
    }
    return wg_group_run<Wg2Group>(descs, g, dw, db, n, plans, pending, stream);
}
extern "C" int msmc_conv_wgrad_group_ws(const msmc_conv_desc* descs, const void* const* g, float* const* dw,
                                        float* const* db, int n, void* workspace, size_t workspace_bytes,
                                        msmc_stream stream) {
    return msmc_conv_wgrad_group_ws4(descs, g, dw, db, n, workspace, workspace_bytes, stream, 0);
}
extern "C" int msmc_conv_wgrad_group(const msmc_conv_desc* descs, const void* const* g, float* const* dw, float* const* db,
                                     int n, msmc_stream stream) {
    return msmc_conv_wgrad_group_ws(descs, g, dw, db, n, nullptr, 0, stream);
}
