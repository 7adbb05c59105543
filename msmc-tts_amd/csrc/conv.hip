// conv.hip -- channels-last implicit-GEMM convolution family for gfx950 (matrix cores): forward and data gradient.
// (weight gradient: conv_wgrad.hip; weight norm, column sums, reflect-fold, leaky-ReLU backward: wnorm.hip)
//
// Replaces the convolutions behind HifiGAN's Generator / ResBlock1
// (reference msmctts/networks/hifigan/generator.py:40-55, common.py:44-51) and the MPD / MRD
// discriminators (reference msmctts/networks/hifigan/discriminator.py:71-76, 135-154).
//
// conv_gather_kernel<T, NT>: out[q][co] = epilogue(sum_t sum_ci W[t][co][ci] * act(x[in(q,t)][ci])).
//   * M = 128 lattice points (a TH x TW block of output pixels of one batch item), N = 32*NT output
//     channels, K = Cin x taps.  4 waves, each a 32 x (32*NT) tile of v_mfma_f32_32x32x16_bf16
//     (bf16 storage) or v_mfma_f32_32x32x2_f32 (fp32 storage: exact fp32, k-ordered fmaf chains).
//   * per 64-byte channel chunk the input halo tile [IH*IW pixels][chunk] is staged ONCE in LDS with the
//     padding rule (zero / reflect) and the input leaky-ReLU applied; every tap then reads its
//     A fragment from the same tile at a shifted row -- the channels-last layout makes a tap a pure
//     row offset, so dilation, stride and 2-D kernels cost nothing extra.
//   * the output lattice (oy0 + qy*osy, ...) and the tap table come from the host, so the same kernel
//     is the forward of strided / dilated convolutions, the forward of transposed convolutions
//     (one launch per output phase) and the data-gradient of all of them.
//   * epilogue in registers: + bias, * leaky-ReLU'(mask_src), + res, res2 + ., / out_div, store
//     (64/128 contiguous bytes per row of the accumulator fragment).
#include <msmc_rt.hpp>
#include <msmc_hip.h>
#include <msmc_hip_debug.h>
#include "conv_common.inc"

extern "C" void msmc_conv_set_pipeline(int on) { msmc_conv_pipeline_enabled = on; }
static int msmc_conv_narrow_when_small = 1;
extern "C" void msmc_conv_set_narrow(int on) { msmc_conv_narrow_when_small = on; }
extern "C" const char* msmc_conv_last_kernel(void) { return msmc_conv_last; }
extern "C" long msmc_conv_launch_count(void) { return msmc_conv_launches; }
extern "C" int msmc_conv_gather(const msmc_conv_desc* d, msmc_stream stream);
static int msmc_gather_generation = 2;          // 1 = first-generation forward / data-gradient kernels (A/B tests)
extern "C" void msmc_conv_set_gather_generation(int n) { msmc_gather_generation = n; }

// Epilogue of N (4 or 8) consecutive bf16 output channels held as floats: mask (leaky-ReLU derivative from the sign of a packed
// bf16 operand), two residuals, division by out_div, output leaky-ReLU.  ONE wave-uniform branch per optional operand around
// all N values: written inside a per-value loop the options were if-converted -- every value paid ~28 vector instructions, an
// 11-instruction IEEE division included, whether or not the operand was there (SQ counters / ISA, round 4: the epilogue was
// 460 of a thin-layer tile's ~740 vector instructions).  The division is a multiplication by the reciprocal (<= 1 ulp in fp32,
// before the bf16 rounding); the fp32 kernels keep the exact division.
template <int N>
MSMC_DEV void cv_ep(float (&v)[N], const unsigned int* mk, const unsigned int* r1, const unsigned int* r2, bool has_mask,
                    bool has_res, bool has_res2, float mslope, float odiv, float oslope) {
    if (has_mask) {
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const float mj = __uint_as_float((j & 1) ? (mk[j >> 1] & 0xffff0000u) : (mk[j >> 1] << 16));
            v[j] = v[j] * (mj > 0.f ? 1.f : mslope);
        }
    }
    if (has_res) {
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] = v[j] + __uint_as_float((j & 1) ? (r1[j >> 1] & 0xffff0000u) : (r1[j >> 1] << 16));
    }
    if (has_res2) {
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] = __uint_as_float((j & 1) ? (r2[j >> 1] & 0xffff0000u) : (r2[j >> 1] << 16)) + v[j];
    }
    if (odiv != 1.f) {
        const float rdiv = 1.f / odiv;
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] = v[j] * rdiv;
    }
    if (oslope != 1.f) {
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] = v[j] > 0.f ? v[j] : v[j] * oslope;
    }
}

// 16 channels of one K-step: A fragment rows = pixels, B fragment rows = output channels.
template <int NT>
MSMC_DEV void mma_chunk16(const float* ap, const float* bp, int bstride32, int g, f32x16 (&acc)[NT]) {
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        f32x4 a4 = *(const f32x4*)(ap + 8 * tt + 4 * g);
        f32x4 b4[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) b4[n] = *(const f32x4*)(bp + n * bstride32 + 8 * tt + 4 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[n] = mfma_f32_32x32x2(a4[e], b4[n][e], acc[n]);
    }
}
template <int NT>
MSMC_DEV void mma_chunk16(const unsigned short* ap, const unsigned short* bp, int bstride32, int g,
                          f32x16 (&acc)[NT]) {
    bf16x8 a = __builtin_bit_cast(bf16x8, *(const u16x8*)(ap + 8 * g));
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        bf16x8 b = __builtin_bit_cast(bf16x8, *(const u16x8*)(bp + n * bstride32 + 8 * g));
        acc[n] = mfma_bf16_32x32x16(a, b, acc[n]);
    }
}

template <typename T, int NT>
__global__ __launch_bounds__(256) void conv_gather_kernel(msmc_conv_desc d, CvGeom G) {
    MSMC_DYN_LDS(smem);
    constexpr int VEC = Elt<T>::VEC, CK = Elt<T>::CK, CKV = CK / VEC, XS = CK + VEC, BN = 32 * NT;
    T* xt = (T*)smem;                       // [IH*IW][XS]
    T* wt = xt + G.xt_elems;                // [ntaps][BN][XS]
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, i = lane & 31, g = lane >> 5;
    int bt = blockIdx.x;
    const int tx_ = bt % G.tilesX;
    bt /= G.tilesX;
    const int ty_ = bt % G.tilesY;
    const int b = bt / G.tilesY;
    const int co0 = blockIdx.y * BN;
    const int qy0 = ty_ * G.TH, qx0 = tx_ * G.TW;
    const int iyBase = qy0 * d.isy + d.iy0 + G.dyMin, ixBase = qx0 * d.isx + d.ix0 + G.dxMin;
    const int IW = G.IW, npix = G.IH * G.IW;

    int arow;
    {
        int m = 32 * w + i;
        int mty = m / G.TW, mtx = m - mty * G.TW;
        arow = (mty < G.TH) ? (mty * d.isy) * IW + mtx * d.isx : 0;
    }
    f32x16 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;

    const T* xb = (const T*)d.x + (size_t)b * d.Hin * d.Win * d.Cin;
    const T* wg = (const T*)d.w;
    const bool vec_ok = (d.Cin % VEC) == 0;
    const float slope = d.in_slope;

    for (int c0 = 0; c0 < d.Cin; c0 += CK) {
        __syncthreads();
        // ---- input halo tile, padding rule and input activation applied once per element
        for (int e = tid; e < npix * CKV; e += 256) {
            const int pi = e / CKV, v = e - pi * CKV;
            const int ry = pi / IW, rx = pi - ry * IW;
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
                if (slope != 1.f) {
#pragma unroll
                    for (int q = 0; q < VEC; ++q) {
                        float f = Elt<T>::ld(&vals[q]);
                        f = f > 0.f ? f : f * slope;
                        Elt<T>::st(&vals[q], f);
                    }
                }
            }
            *(u32x4*)(xt + (size_t)pi * XS + v * VEC) = *(const u32x4*)vals;
        }
        // ---- weight slices of every tap for this channel chunk
        for (int e = tid; e < d.ntaps * BN * CKV; e += 256) {
            const int v = e % CKV;
            const int row = e / CKV;                // t * BN + co_l
            const int t = row / BN, col = row - t * BN;
            const int co = co0 + col, c = c0 + v * VEC;
            alignas(16) T vals[VEC];
#pragma unroll
            for (int q = 0; q < VEC; ++q) vals[q] = 0;
            if (co < d.Cout && c < d.Cin) {
                const T* src = wg + ((size_t)d.tap_w[t] * d.Cout + co) * d.Cin + c;
                if (vec_ok) {
                    *(u32x4*)vals = *(const u32x4*)src;
                } else {
#pragma unroll
                    for (int q = 0; q < VEC; ++q)
                        if (c + q < d.Cin) vals[q] = src[q];
                }
            }
            *(u32x4*)(wt + (size_t)row * XS + v * VEC) = *(const u32x4*)vals;
        }
        __syncthreads();
        for (int t = 0; t < d.ntaps; ++t) {
            const T* ap = xt + (size_t)(arow + (d.tap_dy[t] - G.dyMin) * IW + (d.tap_dx[t] - G.dxMin)) * XS;
            const T* bp = wt + (size_t)(t * BN + i) * XS;
#pragma unroll
            for (int ks = 0; ks < CK / 16; ++ks) mma_chunk16<NT>(ap + ks * 16, bp + ks * 16, 32 * XS, g, acc);
        }
    }

    // ---- epilogue: D fragment reg r -> row (r&3) + 8*(r>>2) + 4*g (pixel), col i (output channel)
    const T* mask = (const T*)d.mask_src;
    const T* res = (const T*)d.res;
    const T* res2 = (const T*)d.res2;
    T* out = (T*)d.out;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int co = co0 + n * 32 + i;
        if (co >= d.Cout) continue;
        const float bv = d.bias ? d.bias[co] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = 32 * w + (r & 3) + 8 * (r >> 2) + 4 * g;
            const int mty = m / G.TW, mtx = m - mty * G.TW;
            const int qy = qy0 + mty, qx = qx0 + mtx;
            if (mty >= G.TH || qy >= d.QH || qx >= d.QW) continue;
            const int oy = d.oy0 + qy * d.osy, ox = d.ox0 + qx * d.osx;
            const size_t o = (((size_t)b * d.Hout + oy) * d.Wout + ox) * d.Cout + co;
            float v = acc[n][r] + bv;
            if (mask) v = v * (Elt<T>::ld(mask + o) > 0.f ? 1.f : d.mask_slope);
            if (res) v = v + Elt<T>::ld(res + o);
            if (res2) v = Elt<T>::ld(res2 + o) + v;
            if (d.out_div != 1.f) v = v / d.out_div;
            if (d.out_slope != 1.f) v = v > 0.f ? v : v * d.out_slope;
            Elt<T>::st(out + o, v);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Pipelined variant: each work-item owns a fixed list of 16-byte staging slots (computed once, so no
// index arithmetic in the K loop); the global loads of channel chunk c+1 are issued into registers
// before the MFMAs of chunk c and written to LDS afterwards, and a wave covers MT 32-row sub-tiles so a
// staged weight chunk is reused MT times (M tile = 128*MT lattice points).
// ------------------------------------------------------------------------------------------------
#define CV_XLD 12
#define CV_WLD 12

template <typename T, int NT, int MT>
__global__ __launch_bounds__(256) void conv_gather_pipe_kernel(msmc_conv_desc d, CvGeom G) {
    MSMC_DYN_LDS(smem);
    constexpr int VEC = Elt<T>::VEC, CK = Elt<T>::CK, CKV = CK / VEC, XS = CK + VEC, BN = 32 * NT;
    T* xt = (T*)smem;
    T* wt = xt + G.xt_elems;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, i = lane & 31, g = lane >> 5;
    int bt = blockIdx.x;
    const int tx_ = bt % G.tilesX;
    bt /= G.tilesX;
    const int ty_ = bt % G.tilesY;
    const int b = bt / G.tilesY;
    const int co0 = blockIdx.y * BN;
    const int qy0 = ty_ * G.TH, qx0 = tx_ * G.TW;
    const int iyBase = qy0 * d.isy + d.iy0 + G.dyMin, ixBase = qx0 * d.isx + d.ix0 + G.dxMin;
    const int IW = G.IW, npix = G.IH * G.IW;
    const T* xb = (const T*)d.x + (size_t)b * d.Hin * d.Win * d.Cin;
    const T* wg = (const T*)d.w;
    const float slope = d.in_slope;

    // ---- staging slots: global element offset (without the chunk base) or -1, and LDS element offset
    long xsrc[CV_XLD], wsrc[CV_WLD];
    int xdst[CV_XLD], wdst[CV_WLD], xch[CV_XLD], wch[CV_WLD];
#pragma unroll
    for (int j = 0; j < CV_XLD; ++j) {
        const int e = tid + 256 * j;
        xsrc[j] = -1; xdst[j] = -1; xch[j] = 0;
        if (e < npix * CKV) {
            const int pi = e / CKV, v = e - pi * CKV;
            const int ry = pi / IW, rx = pi - ry * IW;
            int iy = iyBase + ry, ix = ixBase + rx;
            bool inside = true;
            if (d.pad_mode == 1) {
                iy = reflect_index(iy, d.Hin);
                ix = reflect_index(ix, d.Win);
            } else {
                inside = (iy >= 0) && (iy < d.Hin) && (ix >= 0) && (ix < d.Win);
            }
            xdst[j] = pi * XS + v * VEC;
            xch[j] = v * VEC;
            if (inside) xsrc[j] = ((long)iy * d.Win + ix) * d.Cin + v * VEC;
        }
    }
#pragma unroll
    for (int j = 0; j < CV_WLD; ++j) {
        const int e = tid + 256 * j;
        wsrc[j] = -1; wdst[j] = -1; wch[j] = 0;
        if (e < d.ntaps * BN * CKV) {
            const int v = e % CKV, row = e / CKV;
            const int t = row / BN, col = row - t * BN;
            wdst[j] = row * XS + v * VEC;
            wch[j] = v * VEC;
            if (co0 + col < d.Cout) wsrc[j] = ((long)d.tap_w[t] * d.Cout + co0 + col) * d.Cin + v * VEC;
        }
    }
    int arow[MT];
#pragma unroll
    for (int sI = 0; sI < MT; ++sI) {
        const int m = 32 * (4 * sI + w) + i;
        const int mty = m / G.TW, mtx = m - mty * G.TW;
        arow[sI] = (mty < G.TH) ? (mty * d.isy) * IW + mtx * d.isx : 0;
    }
    f32x16 acc[MT][NT];
#pragma unroll
    for (int sI = 0; sI < MT; ++sI)
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[sI][n][r] = 0.f;

    u32x4 xreg[CV_XLD], wreg[CV_WLD];
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    auto fetch = [&](int c0) {               // Cin % VEC == 0 is guaranteed by the dispatcher
#pragma unroll
        for (int j = 0; j < CV_XLD; ++j) {
            xreg[j] = zero4;
            if (xsrc[j] >= 0 && c0 + xch[j] < d.Cin) xreg[j] = *(const u32x4*)(xb + xsrc[j] + c0);
        }
#pragma unroll
        for (int j = 0; j < CV_WLD; ++j) {
            wreg[j] = zero4;
            if (wsrc[j] >= 0 && c0 + wch[j] < d.Cin) wreg[j] = *(const u32x4*)(wg + wsrc[j] + c0);
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int j = 0; j < CV_XLD; ++j) {
            if (xdst[j] < 0) continue;
            u32x4 v = xreg[j];
            if (slope != 1.f) {
                alignas(16) T vals[VEC];
                *(u32x4*)vals = v;
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    float f = Elt<T>::ld(&vals[q]);
                    f = f > 0.f ? f : f * slope;
                    Elt<T>::st(&vals[q], f);
                }
                v = *(const u32x4*)vals;
            }
            *(u32x4*)(xt + xdst[j]) = v;
        }
#pragma unroll
        for (int j = 0; j < CV_WLD; ++j)
            if (wdst[j] >= 0) *(u32x4*)(wt + wdst[j]) = wreg[j];
    };

    fetch(0);
    for (int c0 = 0; c0 < d.Cin; c0 += CK) {
        __syncthreads();                     // every wave is done reading the previous chunk
        commit();
        __syncthreads();
        if (c0 + CK < d.Cin) fetch(c0 + CK); // in flight during the MFMAs below
        for (int t = 0; t < d.ntaps; ++t) {
            const int toff = (d.tap_dy[t] - G.dyMin) * IW + (d.tap_dx[t] - G.dxMin);
            const T* bp = wt + (size_t)(t * BN + i) * XS;
#pragma unroll
            for (int sI = 0; sI < MT; ++sI) {
                const T* ap = xt + (size_t)(arow[sI] + toff) * XS;
#pragma unroll
                for (int ks = 0; ks < CK / 16; ++ks) mma_chunk16<NT>(ap + ks * 16, bp + ks * 16, 32 * XS, g, acc[sI]);
            }
        }
    }

    const T* mask = (const T*)d.mask_src;
    const T* res = (const T*)d.res;
    const T* res2 = (const T*)d.res2;
    T* out = (T*)d.out;
#pragma unroll
    for (int sI = 0; sI < MT; ++sI)
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int co = co0 + n * 32 + i;
            if (co >= d.Cout) continue;
            const float bv = d.bias ? d.bias[co] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = 32 * (4 * sI + w) + (r & 3) + 8 * (r >> 2) + 4 * g;
                const int mty = m / G.TW, mtx = m - mty * G.TW;
                const int qy = qy0 + mty, qx = qx0 + mtx;
                if (mty >= G.TH || qy >= d.QH || qx >= d.QW) continue;
                const int oy = d.oy0 + qy * d.osy, ox = d.ox0 + qx * d.osx;
                const size_t o = (((size_t)b * d.Hout + oy) * d.Wout + ox) * d.Cout + co;
                float v = acc[sI][n][r] + bv;
                if (mask) v = v * (Elt<T>::ld(mask + o) > 0.f ? 1.f : d.mask_slope);
                if (res) v = v + Elt<T>::ld(res + o);
                if (res2) v = Elt<T>::ld(res2 + o) + v;
                if (d.out_div != 1.f) v = v / d.out_div;
                if (d.out_slope != 1.f) v = v > 0.f ? v : v * d.out_slope;
                Elt<T>::st(out + o, v);
            }
        }
}

// ------------------------------------------------------------------------------------------------
// Second-generation gather kernel.  Same tiling and MFMA schedule as conv_gather_kernel; what changed is
// everything around the matrix cores, which is where the time went (the first generation executed
// ~2000-6000 scalar/vector ALU instructions per work-item around 2-16 MFMAs):
//   * pixel -> global-offset tables for the input halo tile and the output tile are built ONCE per workgroup
//     in LDS (padding rule, reflect, lattice stride and tile raggedness folded in); the channel-chunk loop
//     and the epilogue index them instead of dividing;
//   * the accumulators leave through an fp32 LDS tile, so bias / mask / residual / activation / store
//     run on 16-byte vectors of consecutive channels (one load and one store instruction per 8 bf16)
//     instead of one 2-byte access per element.
// ------------------------------------------------------------------------------------------------
template <typename T, int NT, int CKM, int SB>
MSMC_DEV void cv2_body(const msmc_conv_desc& d, const CvGeom& G, const int block_x, const int block_y) {
    MSMC_DYN_LDS(smem);
    // CKM = 2: 128-byte channel chunks (half the load -> LDS -> MFMA round trips of a deep reduction);
    // SB: weight-slice vectors a work-item keeps in flight per batch (4 or 8)
    constexpr int VEC = Elt<T>::VEC, CK = Elt<T>::CK * CKM, CKV = CK / VEC, XS = CK + VEC, BN = 32 * NT, OS = BN + 4;
    constexpr int BNV = BN / VEC;
    const int npix = G.IH * G.IW, IW = G.IW;
    int* in_off = (int*)smem;                                   // [npix] element offset of halo pixel, -1 = zero
    int* out_off = in_off + npix;                               // [128]  pixel index of lattice point, -1 = none
    int* tapw = out_off + 128;                                  // [16]   weight slice of tap t
    char* region = smem + (((size_t)(npix + 128 + 16) * sizeof(int) + 15) & ~(size_t)15);
    T* xt = (T*)region;                                         // [npix][XS]
    T* wt = xt + (size_t)npix * XS;                             // [ntaps][BN][XS]
    float* ot = (float*)region;                                 // [128][OS] epilogue tile (aliases xt / wt)
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, i = lane & 31, g = lane >> 5;
    int bt = block_x;
    const int tx_ = bt % G.tilesX;
    bt /= G.tilesX;
    const int ty_ = bt % G.tilesY;
    const int b = bt / G.tilesY;
    const int co0 = block_y * BN;
    const int qy0 = ty_ * G.TH, qx0 = tx_ * G.TW;
    const int iyBase = qy0 * d.isy + d.iy0 + G.dyMin, ixBase = qx0 * d.isx + d.ix0 + G.dxMin;

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
    if (tid < 128) {
        const int mty = tid / G.TW, mtx = tid - mty * G.TW;
        const int qy = qy0 + mty, qx = qx0 + mtx;
        const bool valid = mty < G.TH && qy < d.QH && qx < d.QW;
        out_off[tid] = valid ? (d.oy0 + qy * d.osy) * d.Wout + (d.ox0 + qx * d.osx) : -1;
    }
#pragma unroll
    for (int t = 0; t < MSMC_CONV_MAX_TAPS; ++t)
        if (tid == 128 + t) tapw[t] = t < d.ntaps ? d.tap_w[t] : 0;

    int arow;
    {
        const int m = 32 * w + i;
        const int mty = m / G.TW, mtx = m - mty * G.TW;
        arow = (mty < G.TH) ? (mty * d.isy) * IW + mtx * d.isx : 0;
    }
    f32x16 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;

    const T* xb = (const T*)d.x + (size_t)b * d.Hin * d.Win * d.Cin;
    const T* wg = (const T*)d.w;
    const bool vec_ok = (d.Cin % VEC) == 0;
    const float slope = d.in_slope;
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    const int nxv = npix * CKV, nwv = d.ntaps * BN * CKV;

    // staging helpers: loads of a batch are all issued before its LDS stores (one global-load latency per batch)
    auto load_x = [&](int c0, int e0, u32x4 (&vals)[4], int (&dst)[4]) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + 256 * u;
            dst[u] = -1;
            vals[u] = zero4;
            if (e < nxv) {
                const int pi = e / CKV, v = e - pi * CKV;
                const int off = in_off[pi], c = c0 + v * VEC;
                dst[u] = pi * XS + v * VEC;
                if (off >= 0 && c < d.Cin) {
                    const T* src = xb + off + c;
                    if (vec_ok) {
                        vals[u] = *(const u32x4*)src;
                    } else {
                        alignas(16) T tmp[VEC];
#pragma unroll
                        for (int q = 0; q < VEC; ++q) tmp[q] = (c + q < d.Cin) ? src[q] : (T)0;
                        vals[u] = *(const u32x4*)tmp;
                    }
                }
            }
        }
    };
    auto store_x = [&](u32x4 (&vals)[4], int (&dst)[4]) {   // input activation applied once per element
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (dst[u] < 0) continue;
            if (slope != 1.f) {
                if (sizeof(T) == 2 && slope >= 0.f && slope <= 1.f) {      // packed: max(x, slope x) on bf16 pairs, one conversion per pair
#pragma unroll
                    for (int q = 0; q < 4; ++q) vals[u][q] = bf16x2_leaky(vals[u][q], slope);
                } else {
                    alignas(16) T tmp[VEC];
                    *(u32x4*)tmp = vals[u];
#pragma unroll
                    for (int q = 0; q < VEC; ++q) {
                        float f = Elt<T>::ld(&tmp[q]);
                        f = f > 0.f ? f : f * slope;
                        Elt<T>::st(&tmp[q], f);
                    }
                    vals[u] = *(const u32x4*)tmp;
                }
            }
            *(u32x4*)(xt + dst[u]) = vals[u];
        }
    };
    auto load_w = [&](int c0, int e0, u32x4 (&vals)[SB], int (&dst)[SB]) {
#pragma unroll
        for (int u = 0; u < SB; ++u) {
            const int e = e0 + 256 * u;
            dst[u] = -1;
            vals[u] = zero4;
            if (e < nwv) {
                const int row = e / CKV, v = e - row * CKV;       // row = t * BN + output channel
                const int t = row / BN, col = row - t * BN;
                const int co = co0 + col, c = c0 + v * VEC;
                dst[u] = row * XS + v * VEC;
                if (co < d.Cout && c < d.Cin) {
                    const T* src = wg + ((size_t)tapw[t] * d.Cout + co) * d.Cin + c;
                    if (vec_ok) {
                        vals[u] = *(const u32x4*)src;
                    } else {
                        alignas(16) T tmp[VEC];
#pragma unroll
                        for (int q = 0; q < VEC; ++q) tmp[q] = (c + q < d.Cin) ? src[q] : (T)0;
                        vals[u] = *(const u32x4*)tmp;
                    }
                }
            }
        }
    };
    auto store_w = [&](u32x4 (&vals)[SB], int (&dst)[SB]) {
#pragma unroll
        for (int u = 0; u < SB; ++u)
            if (dst[u] >= 0) *(u32x4*)(wt + dst[u]) = vals[u];
    };

    auto mma_taps = [&]() {
        for (int t = 0; t < d.ntaps; ++t) {
            const T* ap = xt + (size_t)(arow + (d.tap_dy[t] - G.dyMin) * IW + (d.tap_dx[t] - G.dxMin)) * XS;
            const T* bp = wt + (size_t)(t * BN + i) * XS;
#pragma unroll
            for (int ks = 0; ks < CK / 16; ++ks) mma_chunk16<NT>(ap + ks * 16, bp + ks * 16, 32 * XS, g, acc);
        }
    };
    if constexpr (SB == 16) {
        // Small grids (about one workgroup per CU, nothing to overlap with): the WHOLE channel chunk -- halo tile and
        // weight slices, up to 16 vectors per work-item -- is in flight at once and the loads of chunk c+1 are issued
        // before the MFMAs of chunk c, so a chunk costs one global-load latency instead of one per 4-vector batch.
        // One index space for the staging vectors: [0, nxv) input halo tile, [nxv, nv) weight slices.
        const int nv = nxv + nwv;
        u32x4 regs[16];
        auto fetch = [&](int c0) {
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int e = u * 256 + tid;
                regs[u] = zero4;
                if (e >= nv) continue;
                const T* src = nullptr;
                int c;
                if (e < nxv) {
                    const int pi = e / CKV;
                    const int off = in_off[pi];
                    c = c0 + (e - pi * CKV) * VEC;
                    if (off >= 0 && c < d.Cin) src = xb + off + c;
                } else {
                    const int e2 = e - nxv;
                    const int row = e2 / CKV;
                    const int t = row / BN, co = co0 + (row - t * BN);
                    c = c0 + (e2 - row * CKV) * VEC;
                    if (co < d.Cout && c < d.Cin) src = wg + ((size_t)tapw[t] * d.Cout + co) * d.Cin + c;
                }
                if (src) regs[u] = *(const u32x4*)src;            // launcher guarantees Cin % VEC == 0 here
            }
        };
        auto commit = [&]() {
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int e = u * 256 + tid;
                if (e >= nv) continue;
                if (e < nxv) {
                    const int pi = e / CKV;
                    u32x4 v = regs[u];
                    if (slope != 1.f) {
                        alignas(16) T tmp[VEC];
                        *(u32x4*)tmp = v;
#pragma unroll
                        for (int q = 0; q < VEC; ++q) {
                            float f = Elt<T>::ld(&tmp[q]);
                            f = f > 0.f ? f : f * slope;
                            Elt<T>::st(&tmp[q], f);
                        }
                        v = *(const u32x4*)tmp;
                    }
                    *(u32x4*)(xt + (size_t)pi * XS + (e - pi * CKV) * VEC) = v;
                } else {
                    const int e2 = e - nxv;
                    const int row = e2 / CKV;
                    *(u32x4*)(wt + (size_t)row * XS + (e2 - row * CKV) * VEC) = regs[u];
                }
            }
        };
        __syncthreads();                                          // offset tables ready
        fetch(0);
        for (int c0 = 0; c0 < d.Cin; c0 += CK) {
            commit();
            __syncthreads();
            if (c0 + CK < d.Cin) fetch(c0 + CK);
            mma_taps();
            __syncthreads();
        }
    } else {
    for (int c0 = 0; c0 < d.Cin; c0 += CK) {
        __syncthreads();                      // tables ready (first pass) / previous chunk's fragments consumed
        {
            // first batch of the halo tile and of the weight slices share one global-load latency
            u32x4 xv[4], wv[SB];
            int xd[4], wd[SB];
            load_x(c0, tid, xv, xd);
            load_w(c0, tid, wv, wd);
            store_x(xv, xd);
            store_w(wv, wd);
        }
        for (int e0 = tid + 1024; e0 < nxv; e0 += 1024) {
            u32x4 xv[4];
            int xd[4];
            load_x(c0, e0, xv, xd);
            store_x(xv, xd);
        }
        for (int e0 = tid + 256 * SB; e0 < nwv; e0 += 256 * SB) {
            u32x4 wv[SB];
            int wd[SB];
            load_w(c0, e0, wv, wd);
            store_w(wv, wd);
        }
        __syncthreads();
        mma_taps();
    }
    }

    // ---- epilogue: accumulators -> fp32 LDS tile -> vectors of VEC consecutive output channels
    __syncthreads();
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            ot[(32 * w + (r & 3) + 8 * (r >> 2) + 4 * g) * OS + n * 32 + i] = acc[n][r];
    __syncthreads();
    const T* mask = (const T*)d.mask_src;
    const T* res = (const T*)d.res;
    const T* res2 = (const T*)d.res2;
    T* out = (T*)d.out;
    const bool ovec = (d.Cout % VEC) == 0;
    const size_t img = (size_t)b * d.Hout * d.Wout;
    for (int e = tid; e < 128 * BNV; e += 256) {
        const int m = e / BNV, vcol = (e - m * BNV) * VEC;
        const int po = out_off[m], co = co0 + vcol;
        if (po < 0 || co >= d.Cout) continue;
        const size_t o = (img + po) * d.Cout + co;
        float v[VEC];
#pragma unroll
        for (int q = 0; q < VEC; ++q) v[q] = ot[m * OS + vcol + q] + ((d.bias && co + q < d.Cout) ? d.bias[co + q] : 0.f);
        alignas(16) T mk[VEC], r1[VEC], r2[VEC], ov[VEC];
        if (ovec) {
            if (mask) *(u32x4*)mk = *(const u32x4*)(mask + o);
            if (res) *(u32x4*)r1 = *(const u32x4*)(res + o);
            if (res2) *(u32x4*)r2 = *(const u32x4*)(res2 + o);
        } else {
#pragma unroll
            for (int q = 0; q < VEC; ++q) {
                const bool in = co + q < d.Cout;
                if (mask) mk[q] = in ? mask[o + q] : (T)0;
                if (res) r1[q] = in ? res[o + q] : (T)0;
                if (res2) r2[q] = in ? res2[o + q] : (T)0;
            }
        }
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
            float x = v[q];
            if (mask) x = x * (Elt<T>::ld(&mk[q]) > 0.f ? 1.f : d.mask_slope);
            if (res) x = x + Elt<T>::ld(&r1[q]);
            if (res2) x = Elt<T>::ld(&r2[q]) + x;
            if (d.out_div != 1.f) x = x / d.out_div;
            if (d.out_slope != 1.f) x = x > 0.f ? x : x * d.out_slope;
            Elt<T>::st(&ov[q], x);
        }
        if (ovec) {
            *(u32x4*)(out + o) = *(const u32x4*)ov;
        } else {
#pragma unroll
            for (int q = 0; q < VEC; ++q)
                if (co + q < d.Cout) out[o + q] = ov[q];
        }
    }
}


template <typename T, int NT, int CKM, int SB>
__global__ __launch_bounds__(256, 2) void conv_gather2_kernel(msmc_conv_desc d, CvGeom G) {
    cv2_body<T, NT, CKM, SB>(d, G, blockIdx.x, blockIdx.y);
}

// Grouped launch: up to MSMC_GROUP_MAX independent convolutions (same kernel instantiation, any geometry) share one
// grid -- the three parallel ResBlocks of a generator stage, the same layer of the five period / six resolution
// sub-discriminators.  Each of them alone is a small grid (tens to a few hundred workgroups) that leaves most of
// the 256 CUs idle at its head and tail; hipGraph branches do not overlap on this stack, one grid does.
struct CvGroupArgs {
    int n;
    int first[MSMC_GROUP_MAX + 1];      // first flattened block of member k (first[n] = total)
    int nx[MSMC_GROUP_MAX];             // blocks along x of member k (flattened id = x + nx * y)
    msmc_conv_desc d[MSMC_GROUP_MAX];
    CvGeom G[MSMC_GROUP_MAX];
};
template <typename T, int NT, int CKM, int SB>
__global__ __launch_bounds__(256, 2) void conv_gather2_group_kernel(CvGroupArgs a) {
    const int k = cv_group_member(a.first, a.n);
    const int id = blockIdx.x - a.first[k];
    cv2_body<T, NT, CKM, SB>(a.d[k], a.G[k], id % a.nx[k], id / a.nx[k]);
}

// ------------------------------------------------------------------------------------------------
// Grouped launch of ONE kernel family (the members of msmc_conv_gather_group it owns).  A family is a traits struct F next
// to its kernel:
//   F::Plan, F::Args        plan of one member (fields applies, lds) / argument block of the family's group kernel
//   F::min_members          members a call must hold before the family groups (fewer: left to the paths after it)
//   F::lone_single          a member left alone in its bucket runs the single kernel here (false: left to the paths after it)
//   F::mine(d)              the member is the family's
//   F::plan(d, pl, share)   plan of one member; share = the family's members in the call, at most MSMC_GROUP_MAX
//   F::same(p, q)           the two plans run one kernel instantiation, so they may share a grid
//   F::blocks(p)            workgroups the member contributes
//   F::head(a, m)           stores the member count, returns first[]
//   F::fill(a, k, d, p)     slot k of the argument block (all of it but first[k])
//   F::dispatch(p, blocks, lds, stream, d, group)      the single kernel on d (group == NULL) or the group kernel; sets
//                           msmc_conv_last
// ------------------------------------------------------------------------------------------------
// fill-and-dispatch step: members[0..m) (plans pl[members[k]], one kernel instantiation) as one launch
template <class F>
static int cv_family_dispatch(const msmc_conv_desc* descs, const typename F::Plan* pl, const int* members, int m,
                              msmc_stream stream) {
    typename F::Args a;
    int* first = F::head(a, m);
    int blocks = 0;
    size_t lds = 0;
    for (int k = 0; k < m; ++k) {
        const int j = members[k];
        first[k] = blocks;
        F::fill(a, k, descs[j], pl[j]);
        blocks += F::blocks(pl[j]);
        if (pl[j].lds > lds) lds = pl[j].lds;
    }
    first[m] = blocks;
    ++msmc_conv_launches;
    return F::dispatch(pl[members[0]], blocks, lds, stream, m == 1 ? &descs[members[0]] : nullptr, m == 1 ? nullptr : &a);
}
// plan every member of the family, bucket the plans that may share a grid (MSMC_GROUP_MAX per launch), launch the buckets in
// member order.  done[i]: launched (here or by a family before this one); a member whose plan does not apply is MSMC_E_SHAPE.
template <class F>
static int cv_family_group_launch(const msmc_conv_desc* descs, int n, msmc_stream stream, bool* done) {
    typename F::Plan pl[MSMC_GROUP_LIMIT];
    bool todo[MSMC_GROUP_LIMIT];
    int count = 0;
    for (int i = 0; i < n; ++i) {
        todo[i] = !done[i] && F::mine(&descs[i]);
        count += todo[i];
    }
    if (count < F::min_members) return 0;
    for (int i = 0; i < n; ++i) {
        if (!todo[i]) continue;
        int rc = F::plan(&descs[i], &pl[i], count < MSMC_GROUP_MAX ? count : MSMC_GROUP_MAX);
        if (rc) return rc;
        if (!pl[i].applies) return MSMC_E_SHAPE;
    }
    for (int i = 0; i < n; ++i) {
        if (!todo[i]) continue;
        int members[MSMC_GROUP_MAX], m = 0;
        for (int j = i; j < n && m < MSMC_GROUP_MAX; ++j) {
            if (!todo[j] || !F::same(pl[i], pl[j])) continue;
            members[m++] = j;
            todo[j] = false;
        }
        if (m == 1 && !F::lone_single) continue;
        for (int k = 0; k < m; ++k) done[members[k]] = true;
        int rc = cv_family_dispatch<F>(descs, pl, members, m, stream);
        if (rc) return rc;
    }
    return 0;
}

#include "gather3.inc"
#include "gather4.inc"
#include "gemm1.inc"
#include "gather5.inc"
#include "gather7.inc"
#include "gather6.inc"

template <typename T, int NT, int MT>
static int cv_try_pipe(const msmc_conv_desc* d, msmc_stream stream, bool* done) {
    constexpr int XS = Elt<T>::CK + Elt<T>::VEC, CKV = Elt<T>::CK / Elt<T>::VEC;
    CvGeom G;
    size_t lds;
    *done = false;
    int rc = cv_geometry(d, &G, sizeof(T), XS, 32 * NT, &lds, CV_BM * MT);
    if (rc) return rc;
    if (lds > 160 * 1024) return 0;
    if (G.IH * G.IW * CKV > 256 * CV_XLD || d->ntaps * 32 * NT * CKV > 256 * CV_WLD) return 0;
    dim3 grid((unsigned)(G.tilesX * G.tilesY * d->B), (unsigned)((d->Cout + 32 * NT - 1) / (32 * NT)));
    rc = msmc_allow_lds((const void*)conv_gather_pipe_kernel<T, NT, MT>, (int)lds);
    if (rc) return rc;
    MSMC_LAUNCH((conv_gather_pipe_kernel<T, NT, MT>), grid, dim3(256), lds, (msmc_stream_t)stream, *d, G);
    msmc_conv_last = msmc_prof_name(msmc_kname("conv_gather_pipe_kernel", EltName<T>::v, NT, MT));
    *done = true;
    return msmc_check_launch();
}

// Kernel choice of the second-generation gather for one descriptor (shared by the single and the grouped launch).
struct Cv2Plan {
    int applies;            // 1: second generation; 0: first-generation dispatch
    int nt, ckm, sb;
    CvGeom G;
    size_t lds;
    unsigned gx, gy;
};
template <typename T>
static int cv2_plan(const msmc_conv_desc* d, Cv2Plan* pl, int* narrow_nt) {
    constexpr int XS = Elt<T>::CK + Elt<T>::VEC;
    pl->applies = 0;
    int NT = d->Cout > 32 ? 2 : 1;
    if (NT == 2 && msmc_conv_narrow_when_small) {
        // few output pixels: 32-channel N tiles double the workgroup count (two co-resident workgroups per CU
        // hide each other's global-load latency, which dominates at this size)
        const long mt = ((long)d->QH * d->QW + CV_BM - 1) / CV_BM * d->B;
        const long wide = mt * ((d->Cout + 63) / 64);
        if (wide < MSMC_NUM_CU || (wide < 2 * MSMC_NUM_CU && d->Cin >= 256)) NT = 1;
    }
    *narrow_nt = NT;
    // second generation for shallow reductions (fewer than 4 channel chunks); deep ones keep the register-prefetching
    // pipelined kernel unless a variant says otherwise: measured per layer on MI355X
    const int gen = d->variant > 0 ? d->variant : msmc_gather_generation;
    const bool sb8 = gen == 4 || gen == 5 || (d->variant == 0 && (long)d->ntaps * 32 * NT * (Elt<T>::CK / Elt<T>::VEC) > 1024);
    const bool ck1 = gen == 3 || gen == 5 || gen == 7;
    const bool want16 = gen == 6 || gen == 7;                  // whole chunk in flight + prefetch (small grids)
    bool shallow = d->Cin < 4 * Elt<T>::CK || (d->Cin % Elt<T>::VEC) != 0 || gen >= 3 || d->variant == 2;
    if (want16 && (d->Cin % Elt<T>::VEC) != 0) return MSMC_E_SHAPE;
    if (!shallow && gen == 2) {
        // heuristic without a tuned variant: deep reductions go to the pipelined kernel only where it would use
        // 256-point (or wider) M tiles, i.e. where it amortises the weight staging over a large grid
        const long points = (long)d->B * d->QH * d->QW;
        const long ntile = (d->Cout + 32 * NT - 1) / (32 * NT);
        shallow = (points / (CV_BM * 2)) * ntile < 2 * MSMC_NUM_CU;
    }
    if (!(gen >= 2 && shallow && (long)d->Hin * d->Win * d->Cin < (1L << 31) && (long)d->Hout * d->Wout < (1L << 31)))
        return 0;
    size_t unused;
    int rc = cv_geometry(d, &pl->G, sizeof(T), XS, 32, &unused);
    if (rc) return rc;
    const long npix = (long)pl->G.IH * pl->G.IW;
    const size_t tables = (((size_t)(npix + 128 + 16) * sizeof(int)) + 15) & ~(size_t)15;
    auto lds_of = [&](int nt, int ckm) {
        const size_t xs = (size_t)Elt<T>::CK * ckm + Elt<T>::VEC;
        const size_t stage = ((size_t)npix + (size_t)d->ntaps * 32 * nt) * xs * sizeof(T);
        const size_t epi = (size_t)128 * (32 * nt + 4) * sizeof(float);
        return tables + (stage > epi ? stage : epi);
    };
    int nt = NT;
    int ckm = (d->Cin >= 2 * Elt<T>::CK && (d->Cin % Elt<T>::VEC) == 0 && lds_of(nt, 2) <= 64 * 1024 && !ck1) ? 2 : 1;
    if (lds_of(nt, ckm) > 160 * 1024 && nt == 2) nt = 1;
    const size_t lds2 = lds_of(nt, ckm);
    const long chunk_vectors = (npix + (long)d->ntaps * 32 * nt) * (Elt<T>::CK * ckm / Elt<T>::VEC);
    const bool sb16 = want16 && chunk_vectors <= 16L * 256 && (d->Cin % Elt<T>::VEC) == 0;
    if (want16 && !sb16) return MSMC_E_SHAPE;                  // the tuner skips candidates that do not apply
    if (lds2 > 160 * 1024) return 0;
    pl->applies = 1;
    pl->nt = nt;
    pl->ckm = ckm;
    pl->sb = sb16 ? 16 : sb8 ? 8 : 4;
    pl->lds = lds2;
    pl->gx = (unsigned)(pl->G.tilesX * pl->G.tilesY * d->B);
    pl->gy = (unsigned)((d->Cout + 32 * nt - 1) / (32 * nt));
    return 0;
}

// the same plan with the tile / chunk / batch parameters imposed (a grouped launch runs ONE instantiation: members
// adopt the parameters of the member with the largest grid when they can)
template <typename T>
static int cv2_plan_forced(const msmc_conv_desc* d, Cv2Plan* pl, int nt, int ckm, int sb) {
    constexpr int XS = Elt<T>::CK + Elt<T>::VEC;
    pl->applies = 0;
    if ((long)d->Hin * d->Win * d->Cin >= (1L << 31) || (long)d->Hout * d->Wout >= (1L << 31)) return 0;
    if (ckm == 2 && (d->Cin < 2 * Elt<T>::CK || (d->Cin % Elt<T>::VEC) != 0)) return 0;
    size_t unused;
    int rc = cv_geometry(d, &pl->G, sizeof(T), XS, 32, &unused);
    if (rc) return rc;
    const long npix = (long)pl->G.IH * pl->G.IW;
    const size_t tables = (((size_t)(npix + 128 + 16) * sizeof(int)) + 15) & ~(size_t)15;
    const size_t xs = (size_t)Elt<T>::CK * ckm + Elt<T>::VEC;
    const size_t stage = ((size_t)npix + (size_t)d->ntaps * 32 * nt) * xs * sizeof(T);
    const size_t epi = (size_t)128 * (32 * nt + 4) * sizeof(float);
    const size_t lds = tables + (stage > epi ? stage : epi);
    if (lds > 160 * 1024) return 0;
    if (sb == 16) {
        const long chunk_vectors = (npix + (long)d->ntaps * 32 * nt) * (Elt<T>::CK * ckm / Elt<T>::VEC);
        if (chunk_vectors > 16L * 256 || (d->Cin % Elt<T>::VEC) != 0) return 0;
    }
    pl->applies = 1;
    pl->nt = nt;
    pl->ckm = ckm;
    pl->sb = sb;
    pl->lds = lds;
    pl->gx = (unsigned)(pl->G.tilesX * pl->G.tilesY * d->B);
    pl->gy = (unsigned)((d->Cout + 32 * nt - 1) / (32 * nt));
    return 0;
}

// launch one second-generation kernel instantiation: SINGLE (desc, geometry) or GROUP (CvGroupArgs)
#define CV2_INST(T_, NT_, CKM_, SB_, GROUP_, ...)                                                                  \
    do {                                                                                                           \
        if (GROUP_) {                                                                                              \
            rc = msmc_allow_lds((const void*)conv_gather2_group_kernel<T_, NT_, CKM_, SB_>, (int)lds);             \
            if (rc) return rc;                                                                                     \
            MSMC_LAUNCH((conv_gather2_group_kernel<T_, NT_, CKM_, SB_>), grid, dim3(256), lds,                     \
                        (msmc_stream_t)stream, *group);                                                            \
        } else {                                                                                                   \
            rc = msmc_allow_lds((const void*)conv_gather2_kernel<T_, NT_, CKM_, SB_>, (int)lds);                   \
            if (rc) return rc;                                                                                     \
            MSMC_LAUNCH((conv_gather2_kernel<T_, NT_, CKM_, SB_>), grid, dim3(256), lds, (msmc_stream_t)stream,    \
                        *d, *G);                                                                                   \
        }                                                                                                          \
    } while (0)
template <typename T>
static int cv2_dispatch(int nt, int ckm, int sb, dim3 grid, size_t lds, msmc_stream stream, const msmc_conv_desc* d,
                        const CvGeom* G, const CvGroupArgs* group) {
    int rc;
    const bool grp = group != nullptr;
#define CV2_SB(NT_, CKM_)                                                                                          \
    do {                                                                                                           \
        if (sb == 16) CV2_INST(T, NT_, CKM_, 16, grp);                                                             \
        else if (sb == 8) CV2_INST(T, NT_, CKM_, 8, grp);                                                          \
        else CV2_INST(T, NT_, CKM_, 4, grp);                                                                       \
    } while (0)
    if (nt == 2 && ckm == 2) CV2_SB(2, 2);
    else if (nt == 2) CV2_SB(2, 1);
    else if (ckm == 2) CV2_SB(1, 2);
    else CV2_SB(1, 1);
#undef CV2_SB
    msmc_conv_last = msmc_prof_name(msmc_kname2(grp ? "conv_gather2_group_kernel" : "conv_gather2_kernel", EltName<T>::v, nt, ckm, sb));
    return msmc_check_launch();
}
// fill-and-dispatch of second-generation members that share a grid (cv_family_dispatch); which members do is decided by
// cv_group_launch: they adopt the plan of the member with the largest grid
template <typename T>
struct Cv2Family {
    typedef Cv2Plan Plan;
    typedef CvGroupArgs Args;
    static bool same(const Plan& p, const Plan& q) { return p.nt == q.nt && p.ckm == q.ckm && p.sb == q.sb; }
    static int blocks(const Plan& p) { return (int)(p.gx * p.gy); }
    static int* head(Args& a, int m) { a.n = m; return a.first; }
    static void fill(Args& a, int k, const msmc_conv_desc& d, const Plan& p) {
        a.nx[k] = (int)p.gx;
        a.d[k] = d;
        a.G[k] = p.G;
    }
    static int dispatch(const Plan& p, int blocks, size_t lds, msmc_stream stream, const msmc_conv_desc* d, const Args* group) {
        return cv2_dispatch<T>(p.nt, p.ckm, p.sb, group ? dim3((unsigned)blocks) : dim3(p.gx, p.gy), lds, stream, d, &p.G, group);
    }
};

template <typename T>
static int cv_launch(const msmc_conv_desc* d, msmc_stream stream) {
    constexpr int XS = Elt<T>::CK + Elt<T>::VEC;
    Cv2Plan pl;
    int NT;
    int rc0 = cv2_plan<T>(d, &pl, &NT);
    if (rc0) return rc0;
    if (pl.applies)
        return cv2_dispatch<T>(pl.nt, pl.ckm, pl.sb, dim3(pl.gx, pl.gy), pl.lds, stream, d, &pl.G, nullptr);
    // the pipelined kernel pays a slot-table prologue: worth it from ~4 channel chunks on (measured per layer)
    const bool deep = d->Cin >= 4 * Elt<T>::CK || msmc_conv_pipeline_enabled >= 2;
    if ((d->Cin % Elt<T>::VEC) == 0 && msmc_conv_pipeline_enabled && deep) {
        // widest M tile that still leaves >= ~2 workgroups per CU
        const long points = (long)d->B * d->QH * d->QW;
        const long ntile = (d->Cout + 32 * NT - 1) / (32 * NT);
        int MT = 4;
        if (msmc_conv_pipeline_enabled == 2 || msmc_conv_pipeline_enabled == 4) MT = msmc_conv_pipeline_enabled;   // tests
        else while (MT > 1 && (points / (CV_BM * MT)) * ntile < 2 * MSMC_NUM_CU) MT >>= 1;
        bool done = false;
        int rc = 0;
        for (; MT >= 1 && !done; MT >>= 1) {
            if (NT == 2) {
                if (MT == 4) rc = cv_try_pipe<T, 2, 4>(d, stream, &done);
                else if (MT == 2) rc = cv_try_pipe<T, 2, 2>(d, stream, &done);
                else rc = cv_try_pipe<T, 2, 1>(d, stream, &done);
            } else {
                if (MT == 4) rc = cv_try_pipe<T, 1, 4>(d, stream, &done);
                else if (MT == 2) rc = cv_try_pipe<T, 1, 2>(d, stream, &done);
                else rc = cv_try_pipe<T, 1, 1>(d, stream, &done);
            }
            if (rc) return rc;
        }
        if (done) return 0;
    }
    CvGeom G;
    size_t lds;
    int rc = cv_geometry(d, &G, sizeof(T), XS, 32 * NT, &lds);
    if (rc) return rc;
    if (lds > 160 * 1024 && NT == 2) {
        NT = 1;
        rc = cv_geometry(d, &G, sizeof(T), XS, 32, &lds);
        if (rc) return rc;
    }
    if (lds > 160 * 1024) return MSMC_E_SHAPE;
    dim3 grid((unsigned)(G.tilesX * G.tilesY * d->B), (unsigned)((d->Cout + 32 * NT - 1) / (32 * NT)));
    if (NT == 2) {
        rc = msmc_allow_lds((const void*)conv_gather_kernel<T, 2>, (int)lds);
        if (rc) return rc;
        MSMC_LAUNCH((conv_gather_kernel<T, 2>), grid, dim3(256), lds, (msmc_stream_t)stream, *d, G);
        msmc_conv_last = msmc_prof_name(msmc_kname("conv_gather_kernel", EltName<T>::v, 2, -1));
    } else {
        rc = msmc_allow_lds((const void*)conv_gather_kernel<T, 1>, (int)lds);
        if (rc) return rc;
        MSMC_LAUNCH((conv_gather_kernel<T, 1>), grid, dim3(256), lds, (msmc_stream_t)stream, *d, G);
        msmc_conv_last = msmc_prof_name(msmc_kname("conv_gather_kernel", EltName<T>::v, 1, -1));
    }
    return msmc_check_launch();
}

// ------------------------------------------------------------------------------------------------
// Direct (matrix-core-free) kernels for the layers an MFMA tile cannot fill: the first discriminator layers
// (2 -> 4 .. 8 -> 16 channels), the score layers (C -> 1) and their data gradients (1 -> C).  They are a few MB of
// memory traffic each; a 128 x 32 MFMA tile spends its time staging 64-byte channel chunks that are 87-97 % padding.
//   small: one work-item per lattice point, all (<= 16) output channels in registers, weights as floats in LDS
//   dot  : one wave per lattice point, lanes over 16-byte channel vectors, butterfly reduction      (Cout == 1)
//   outer: one work-item per (lattice point, 16-byte vector of output channels)                      (Cin == 1)
// Same descriptor semantics (lattice, taps, padding rule, input activation, epilogue) as conv_gather_kernel.
// ------------------------------------------------------------------------------------------------
struct DirPoint {
    int b, qy, qx;
    size_t out;                 // element offset of the output pixel's channel 0
};
MSMC_DEV DirPoint dir_point(const msmc_conv_desc& d, long p) {
    DirPoint r;
    const int per = d.QH * d.QW;
    r.b = (int)(p / per);
    const int rem = (int)(p - (long)r.b * per);
    r.qy = rem / d.QW;
    r.qx = rem - r.qy * d.QW;
    r.out = (((size_t)r.b * d.Hout + (d.oy0 + r.qy * d.osy)) * d.Wout + (d.ox0 + r.qx * d.osx)) * d.Cout;
    return r;
}
// element offset of input pixel (channel 0) for tap t of a point, or -1 when the tap reads zero padding
MSMC_DEV long dir_in(const msmc_conv_desc& d, const DirPoint& pt, int t) {
    int iy = pt.qy * d.isy + d.iy0 + d.tap_dy[t], ix = pt.qx * d.isx + d.ix0 + d.tap_dx[t];
    if (d.pad_mode == 1) {
        iy = reflect_index(iy, d.Hin);
        ix = reflect_index(ix, d.Win);
    } else if (iy < 0 || iy >= d.Hin || ix < 0 || ix >= d.Win) {
        return -1;
    }
    return (((long)pt.b * d.Hin + iy) * d.Win + ix) * d.Cin;
}
template <typename T>
MSMC_DEV float dir_epilogue(const msmc_conv_desc& d, float v, size_t o, int co) {
    if (d.bias) v = v + d.bias[co];
    if (d.mask_src) v = v * (Elt<T>::ld((const T*)d.mask_src + o) > 0.f ? 1.f : d.mask_slope);
    if (d.res) v = v + Elt<T>::ld((const T*)d.res + o);
    if (d.res2) v = Elt<T>::ld((const T*)d.res2 + o) + v;
    if (d.out_div != 1.f) v = v / d.out_div;
    if (d.out_slope != 1.f) v = v > 0.f ? v : v * d.out_slope;
    return v;
}
MSMC_DEV float dir_act(float f, float slope) { return (slope == 1.f || f > 0.f) ? f : f * slope; }

// A run of N consecutive output channels (N * sizeof(T) = 8 bytes or a multiple of 16, the run aligned to its size): the optional operands
// arrive as ONE vector load each and the result leaves as one vector store per 16 bytes -- written per element (dir_epilogue in a
// loop, Elt::st per channel) every work-item issued N two-byte loads per operand and N two-byte stores, each a memory request
// of its own (round 6: the thin first / last layers of the discriminators ran at 7-12 % of the HBM roofline).  Same arithmetic, in
// the same order, as dir_epilogue.
template <typename T, int N>
MSMC_DEV void dir_epilogue_run(const msmc_conv_desc& d, float (&v)[N], const size_t o, const int co0) {
    constexpr int BYTES = N * (int)sizeof(T);
    static_assert(BYTES % 16 == 0 || BYTES == 8, "vector run");
    alignas(16) T mk[N], r1[N], r2[N], ov[N];
    auto ldrun = [&](const T* src, T (&dst)[N]) {
        if constexpr (BYTES % 16 == 0) {
#pragma unroll
            for (int q = 0; q < BYTES / 16; ++q) ((u32x4*)dst)[q] = ((const u32x4*)(src + o))[q];
        } else {
            *(u32x2*)dst = *(const u32x2*)(src + o);
        }
    };
    if (d.bias) {
#pragma unroll
        for (int q = 0; q < N; ++q) v[q] = v[q] + d.bias[co0 + q];
    }
    if (d.mask_src) {
        ldrun((const T*)d.mask_src, mk);
#pragma unroll
        for (int q = 0; q < N; ++q) v[q] = v[q] * (Elt<T>::ld(&mk[q]) > 0.f ? 1.f : d.mask_slope);
    }
    if (d.res) {
        ldrun((const T*)d.res, r1);
#pragma unroll
        for (int q = 0; q < N; ++q) v[q] = v[q] + Elt<T>::ld(&r1[q]);
    }
    if (d.res2) {
        ldrun((const T*)d.res2, r2);
#pragma unroll
        for (int q = 0; q < N; ++q) v[q] = Elt<T>::ld(&r2[q]) + v[q];
    }
    if (d.out_div != 1.f) {
#pragma unroll
        for (int q = 0; q < N; ++q) v[q] = v[q] / d.out_div;
    }
    if (d.out_slope != 1.f) {
#pragma unroll
        for (int q = 0; q < N; ++q) v[q] = v[q] > 0.f ? v[q] : v[q] * d.out_slope;
    }
#pragma unroll
    for (int q = 0; q < N; ++q) Elt<T>::st(&ov[q], v[q]);
    T* out = (T*)d.out + o;
    if constexpr (BYTES % 16 == 0) {
#pragma unroll
        for (int q = 0; q < BYTES / 16; ++q) ((u32x4*)out)[q] = ((const u32x4*)ov)[q];
    } else {
        *(u32x2*)out = *(const u32x2*)ov;
    }
}

template <typename T, int CI, int CO>
MSMC_DEV void dir_small_body(const msmc_conv_desc& d, const long npoints, const int block, const int nblocks) {
    MSMC_DYN_LDS(smem);
    float* wl = (float*)smem;                       // [ntaps][CI][CO], zero beyond the real channels
    for (int e = threadIdx.x; e < d.ntaps * CI * CO; e += 256) {
        const int co = e % CO, ci = (e / CO) % CI, t = e / (CO * CI);
        float v = 0.f;
        if (co < d.Cout && ci < d.Cin) v = Elt<T>::ld((const T*)d.w + ((size_t)d.tap_w[t] * d.Cout + co) * d.Cin + ci);
        wl[e] = v;
    }
    __syncthreads();
    const T* x = (const T*)d.x;
    T* out = (T*)d.out;
    for (long p = (long)block * 256 + threadIdx.x; p < npoints; p += (long)nblocks * 256) {
        const DirPoint pt = dir_point(d, p);
        float acc[CO];
#pragma unroll
        for (int co = 0; co < CO; ++co) acc[co] = 0.f;
        // (the input vectors of three taps are requested together -- taps outside the image re-read the point's first pixel and are
        //  skipped in the sum -- instead of one memory round trip per tap)
        for (int t0 = 0; t0 < d.ntaps; t0 += 3) {
            alignas(16) T xv[3][CI];
            bool on[3];
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const long off_ = t0 + u < d.ntaps ? dir_in(d, pt, t0 + u) : -1;
                on[u] = off_ >= 0;
                const long off = on[u] ? off_ : 0;
                if (CI * sizeof(T) == 16 && d.Cin == CI) {
                    *(u32x4*)xv[u] = *(const u32x4*)(x + off);
                } else if (CI * sizeof(T) == 8 && d.Cin == CI) {
                    *(u32x2*)xv[u] = *(const u32x2*)(x + off);
                } else if (CI * sizeof(T) == 4 && d.Cin == CI) {
                    *(unsigned int*)xv[u] = *(const unsigned int*)(x + off);
                } else {
#pragma unroll
                    for (int ci = 0; ci < CI; ++ci) xv[u][ci] = ci < d.Cin ? x[off + ci] : (T)0;
                }
            }
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                if (!on[u]) continue;
                const float* wt = wl + (t0 + u) * CI * CO;
#pragma unroll
                for (int ci = 0; ci < CI; ++ci) {
                    const float xf = dir_act(Elt<T>::ld(&xv[u][ci]), d.in_slope);
#pragma unroll
                    for (int co = 0; co < CO; ++co) acc[co] = fmaf(wt[ci * CO + co], xf, acc[co]);
                }
            }
        }
        if constexpr ((CO * sizeof(T)) % 8 == 0) {
            if (d.Cout == CO) {                     // (the whole channel run of the point: vector operands, vector store)
                dir_epilogue_run<T, CO>(d, acc, pt.out, 0);
                continue;
            }
        }
#pragma unroll
        for (int co = 0; co < CO; ++co)
            if (co < d.Cout) Elt<T>::st(out + pt.out + co, dir_epilogue<T>(d, acc[co], pt.out + co, co));
    }
}

struct DirGroupArgs {
    int n;
    int first[MSMC_GROUP_MAX + 1];
    long items[MSMC_GROUP_MAX];         // lattice points (small, dot) or point x vector items (outer) of member k
    msmc_conv_desc d[MSMC_GROUP_MAX];
};
template <typename T, int CI, int CO>
__global__ __launch_bounds__(256) void conv_direct_small_kernel(msmc_conv_desc d, long npoints) {
    dir_small_body<T, CI, CO>(d, npoints, blockIdx.x, gridDim.x);
}
template <typename T, int CI, int CO>
__global__ __launch_bounds__(256) void conv_direct_small_group_kernel(DirGroupArgs a) {
    const int k = cv_group_member(a.first, a.n);
    dir_small_body<T, CI, CO>(a.d[k], a.items[k], blockIdx.x - a.first[k], a.first[k + 1] - a.first[k]);
}

template <typename T>
MSMC_DEV void dir_dot_body(const msmc_conv_desc& d, const long npoints, const int block, const int nblocks) {
    MSMC_DYN_LDS(smem);
    constexpr int VEC = Elt<T>::VEC;
    T* wl = (T*)smem;                               // [ntaps][Cin]
    const int nvec = d.Cin / VEC;
    for (int e = threadIdx.x; e < d.ntaps * nvec; e += 256) {
        const int t = e / nvec, v = e - t * nvec;
        *(u32x4*)(wl + (size_t)t * d.Cin + v * VEC) = *(const u32x4*)((const T*)d.w + (size_t)d.tap_w[t] * d.Cin + v * VEC);
    }
    __syncthreads();
    const T* x = (const T*)d.x;
    T* out = (T*)d.out;
    const int lane = threadIdx.x & 63;
    const long wave = (long)block * 4 + (threadIdx.x >> 6), nwaves = (long)nblocks * 4;
    for (long p = wave; p < npoints; p += nwaves) {
        const DirPoint pt = dir_point(d, p);
        float acc = 0.f;
        for (int t = 0; t < d.ntaps; ++t) {
            const long off = dir_in(d, pt, t);
            if (off < 0) continue;
            for (int v = lane; v < nvec; v += 64) {
                alignas(16) T xv[VEC], wv[VEC];
                *(u32x4*)xv = *(const u32x4*)(x + off + v * VEC);
                *(u32x4*)wv = *(const u32x4*)(wl + (size_t)t * d.Cin + v * VEC);
#pragma unroll
                for (int q = 0; q < VEC; ++q)
                    acc = fmaf(Elt<T>::ld(&wv[q]), dir_act(Elt<T>::ld(&xv[q]), d.in_slope), acc);
            }
        }
        for (int m = 1; m < 64; m <<= 1) acc = acc + wave_xor(acc, m);
        if (lane == 0) Elt<T>::st(out + pt.out, dir_epilogue<T>(d, acc, pt.out, 0));
    }
}

template <typename T>
__global__ __launch_bounds__(256) void conv_direct_dot_kernel(msmc_conv_desc d, long npoints) {
    dir_dot_body<T>(d, npoints, blockIdx.x, gridDim.x);
}
template <typename T>
__global__ __launch_bounds__(256) void conv_direct_dot_group_kernel(DirGroupArgs a) {
    const int k = cv_group_member(a.first, a.n);
    dir_dot_body<T>(a.d[k], a.items[k], blockIdx.x - a.first[k], a.first[k + 1] - a.first[k]);
}

template <typename T>
MSMC_DEV void dir_outer_body(const msmc_conv_desc& d, const long nitems, const int block, const int nblocks) {
    MSMC_DYN_LDS(smem);
    constexpr int VEC = Elt<T>::VEC;
    T* wl = (T*)smem;                               // [ntaps][Cout]   (Cin == 1)
    const int nvec = d.Cout / VEC;
    for (int e = threadIdx.x; e < d.ntaps * nvec; e += 256) {
        const int t = e / nvec, v = e - t * nvec;
        *(u32x4*)(wl + (size_t)t * d.Cout + v * VEC) = *(const u32x4*)((const T*)d.w + (size_t)d.tap_w[t] * d.Cout + v * VEC);
    }
    __syncthreads();
    const T* x = (const T*)d.x;
    T* out = (T*)d.out;
    for (long it = (long)block * 256 + threadIdx.x; it < nitems; it += (long)nblocks * 256) {
        const long p = it / nvec;
        const int v = (int)(it - p * nvec);
        const DirPoint pt = dir_point(d, p);
        float acc[VEC];
#pragma unroll
        for (int q = 0; q < VEC; ++q) acc[q] = 0.f;
        // the input values of four taps at a time: requested together (taps outside the image re-read element 0 and are skipped
        // in the sum, as before) -- one memory round trip per four taps instead of one per tap
        for (int t0 = 0; t0 < d.ntaps; t0 += 4) {
            float xf[4];
            bool on[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long off = t0 + u < d.ntaps ? dir_in(d, pt, t0 + u) : -1;
                on[u] = off >= 0;
                xf[u] = Elt<T>::ld(x + (on[u] ? off : 0));
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (!on[u]) continue;
                const float xa = dir_act(xf[u], d.in_slope);
                alignas(16) T wv[VEC];
                *(u32x4*)wv = *(const u32x4*)(wl + (size_t)(t0 + u) * d.Cout + v * VEC);
#pragma unroll
                for (int q = 0; q < VEC; ++q) acc[q] = fmaf(Elt<T>::ld(&wv[q]), xa, acc[q]);
            }
        }
        dir_epilogue_run<T, VEC>(d, acc, pt.out + (size_t)v * VEC, v * VEC);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void conv_direct_outer_kernel(msmc_conv_desc d, long nitems) {
    dir_outer_body<T>(d, nitems, blockIdx.x, gridDim.x);
}
template <typename T>
__global__ __launch_bounds__(256) void conv_direct_outer_group_kernel(DirGroupArgs a) {
    const int k = cv_group_member(a.first, a.n);
    dir_outer_body<T>(a.d[k], a.items[k], blockIdx.x - a.first[k], a.first[k + 1] - a.first[k]);
}

// returns 1 when a direct kernel was launched, 0 when none applies, < 0 on error
template <typename T>
static int cv_direct_launch(const msmc_conv_desc* d, msmc_stream stream) {
    constexpr int VEC = Elt<T>::VEC;
    const long npoints = (long)d->B * d->QH * d->QW;
    auto blocks = [](long items) {
        long b = (items + 255) / 256;
        const long cap = 16L * MSMC_NUM_CU;
        return (unsigned)(b < 1 ? 1 : b > cap ? cap : b);
    };
    int rc;
    if (d->Cin <= 8 && d->Cout <= 16 && !(d->Cin == 1 && d->Cout % VEC == 0 && d->Cout >= 4 * VEC)) {
        const int CI = d->Cin <= 1 ? 1 : d->Cin <= 2 ? 2 : d->Cin <= 4 ? 4 : 8;
        const int CO = d->Cout <= 1 ? 1 : d->Cout <= 4 ? 4 : d->Cout <= 8 ? 8 : 16;
        const size_t lds = (size_t)d->ntaps * CI * CO * sizeof(float);
#define DIR_GO(CI_, CO_)                                                                                            \
    do {                                                                                                            \
        rc = msmc_allow_lds((const void*)conv_direct_small_kernel<T, CI_, CO_>, (int)lds);                          \
        if (rc) return rc;                                                                                          \
        MSMC_LAUNCH((conv_direct_small_kernel<T, CI_, CO_>), dim3(blocks(npoints)), dim3(256), lds,                 \
                    (msmc_stream_t)stream, *d, npoints);                                                            \
    } while (0)
#define DIR_CO(CI_)                                                                                                 \
    do {                                                                                                            \
        if (CO == 1) DIR_GO(CI_, 1);                                                                                \
        else if (CO == 4) DIR_GO(CI_, 4);                                                                           \
        else if (CO == 8) DIR_GO(CI_, 8);                                                                           \
        else DIR_GO(CI_, 16);                                                                                       \
    } while (0)
        if (CI == 1) DIR_CO(1);
        else if (CI == 2) DIR_CO(2);
        else if (CI == 4) DIR_CO(4);
        else DIR_CO(8);
#undef DIR_CO
#undef DIR_GO
        msmc_conv_last = msmc_prof_name(msmc_kname2("conv_direct_small_kernel", EltName<T>::v, CI, CO, 0));
        rc = msmc_check_launch();
        return rc ? rc : 1;
    }
    if (d->Cout == 1 && d->Cin % VEC == 0 && d->Cin >= 8 * VEC) {
        const size_t lds = (size_t)d->ntaps * d->Cin * sizeof(T);
        if (lds > 160 * 1024) return 0;
        rc = msmc_allow_lds((const void*)conv_direct_dot_kernel<T>, (int)lds);
        if (rc) return rc;
        long b = (npoints + 3) / 4;
        if (b > 8L * MSMC_NUM_CU) b = 8L * MSMC_NUM_CU;
        MSMC_LAUNCH((conv_direct_dot_kernel<T>), dim3((unsigned)(b < 1 ? 1 : b)), dim3(256), lds, (msmc_stream_t)stream, *d,
                    npoints);
        msmc_conv_last = msmc_prof_name(msmc_kname("conv_direct_dot_kernel", EltName<T>::v, 0, -1));
        rc = msmc_check_launch();
        return rc ? rc : 1;
    }
    if (d->Cin == 1 && d->Cout % VEC == 0) {
        const size_t lds = (size_t)d->ntaps * d->Cout * sizeof(T);
        if (lds > 160 * 1024) return 0;
        const long nitems = npoints * (d->Cout / VEC);
        rc = msmc_allow_lds((const void*)conv_direct_outer_kernel<T>, (int)lds);
        if (rc) return rc;
        MSMC_LAUNCH((conv_direct_outer_kernel<T>), dim3(blocks(nitems)), dim3(256), lds, (msmc_stream_t)stream, *d, nitems);
        msmc_conv_last = msmc_prof_name(msmc_kname("conv_direct_outer_kernel", EltName<T>::v, 0, -1));
        rc = msmc_check_launch();
        return rc ? rc : 1;
    }
    return 0;
}

template <typename T>
static int cv_ks_launch(const msmc_conv_desc* d, msmc_stream stream);

extern "C" int msmc_conv_gather(const msmc_conv_desc* d, msmc_stream stream) {
    if (!d || !cv_desc_ok(d)) return MSMC_E_SHAPE;
    ++msmc_conv_launches;
    // variant 8 = direct kernels (E_SHAPE when none applies); without a tuned variant they are the default for the
    // layers they cover (generation 1 keeps the MFMA kernels everywhere: A/B tests)
    if (d->variant == 8 || (d->variant == 0 && msmc_gather_generation >= 2)) {
        int rc = d->dtype == 0 ? cv_direct_launch<float>(d, stream)
                 : d->dtype == 1 ? cv_direct_launch<unsigned short>(d, stream) : MSMC_E_SHAPE;
        if (rc != 0) return rc < 0 ? rc : 0;
        if (d->variant == 8) return MSMC_E_SHAPE;
    }
    // bf16 kernel families chosen by variant, in this order: third generation, persistent thin-layer kernel, 1-tap layers as
    // a plain channel GEMM, fifth generation (sixteen waves, staged taps), seventh generation (eight waves of 64 x 64, two
    // workgroups per CU), thin-channel kernel (fragments straight from global memory).  E_SHAPE outside a family's scope.
    static const struct {
        bool (*is_variant)(int);
        int (*launch)(const msmc_conv_desc*, msmc_stream);
    } families[] = {{cv3_is_variant, cv3_launch}, {cv4_is_variant, cv4_launch}, {g1_is_variant, g1_launch},
                    {cv5_is_variant, cv5_launch}, {cv7_is_variant, cv7_launch}, {cv6_is_variant, cv6_launch}};
    for (const auto& f : families) {
        if (!f.is_variant(d->variant)) continue;
        const int rc = f.launch(d, stream);
        return rc < 0 ? rc : rc == 1 ? 0 : MSMC_E_SHAPE;
    }
    if (d->variant == 9) {                      // wave-split deep reduction (E_SHAPE when it does not apply)
        int rc = d->dtype == 0 ? cv_ks_launch<float>(d, stream)
                 : d->dtype == 1 ? cv_ks_launch<unsigned short>(d, stream) : MSMC_E_SHAPE;
        return rc < 0 ? rc : rc == 1 ? 0 : MSMC_E_SHAPE;
    }
    if (d->dtype == 0) return cv_launch<float>(d, stream);
    if (d->dtype == 1) return cv_launch<unsigned short>(d, stream);
    return MSMC_E_SHAPE;
}

// ------------------------------------------------------------------------------------------------
// Deep reductions on small grids (FFT-block convolutions at T/4, conv_pre, the deep MPD / MRD layers): the 128-point
// kernels leave most CUs idle and walk 16-38 dependent channel-chunk round trips.  Here a workgroup owns 32 lattice
// points x BN channels and its four waves split the channel chunks (wave w takes chunks w, w+4, ...), each staging
// into its own LDS region with wave-level hand-offs only; the four partial tiles meet in LDS before the epilogue.
// Four times the workgroups, a quarter of the chain.
// ------------------------------------------------------------------------------------------------
template <typename T, int NT, int CKM>
MSMC_DEV void cvks_body(const msmc_conv_desc& d, const CvGeom& G, const int region_bytes, const int block_x, const int block_y) {
    MSMC_DYN_LDS(smem);
    constexpr int VEC = Elt<T>::VEC, CK = Elt<T>::CK * CKM, CKV = CK / VEC, XS = CK + VEC, BN = 32 * NT, OS = BN + 4;
    constexpr int BNV = BN / VEC, SB = 8;
    const int npix = G.IH * G.IW, IW = G.IW;
    int* in_off = (int*)smem;                                   // [npix]
    int* out_off = in_off + npix;                               // [32]
    int* tapw = out_off + 32;                                   // [16]
    char* regions = smem + (((size_t)(npix + 32 + 16) * sizeof(int) + 15) & ~(size_t)15);
    const int tid = threadIdx.x, w = wave_uniform(tid >> 6), lane = tid & 63, i = lane & 31, g = lane >> 5;
    T* xt = (T*)(regions + (size_t)w * region_bytes);           // this wave's [npix][XS]
    T* wt = xt + (size_t)npix * XS;                             //             [ntaps][BN][XS]
    int bt = block_x;
    const int tx_ = bt % G.tilesX;
    bt /= G.tilesX;
    const int ty_ = bt % G.tilesY;
    const int b = bt / G.tilesY;
    const int co0 = block_y * BN;
    const int qy0 = ty_ * G.TH, qx0 = tx_ * G.TW;
    const int iyBase = qy0 * d.isy + d.iy0 + G.dyMin, ixBase = qx0 * d.isx + d.ix0 + G.dxMin;
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
    if (tid < 32) {
        const int mty = tid / G.TW, mtx = tid - mty * G.TW;
        const int qy = qy0 + mty, qx = qx0 + mtx;
        const bool valid = mty < G.TH && qy < d.QH && qx < d.QW;
        out_off[tid] = valid ? (d.oy0 + qy * d.osy) * d.Wout + (d.ox0 + qx * d.osx) : -1;
    }
#pragma unroll
    for (int t = 0; t < MSMC_CONV_MAX_TAPS; ++t)
        if (tid == 64 + t) tapw[t] = t < d.ntaps ? d.tap_w[t] : 0;
    int arow;
    {
        const int mty = i / G.TW, mtx = i - mty * G.TW;
        arow = (mty < G.TH) ? (mty * d.isy) * IW + mtx * d.isx : 0;
    }
    f32x16 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
    const T* xb = (const T*)d.x + (size_t)b * d.Hin * d.Win * d.Cin;
    const T* wg = (const T*)d.w;
    const float slope = d.in_slope;
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    const int nxv = npix * CKV, nwv = d.ntaps * BN * CKV;
    __syncthreads();                                            // offset tables ready

    for (int c0 = w * CK; c0 < d.Cin; c0 += 4 * CK) {
        for (int e0 = lane; e0 < nxv; e0 += 64 * SB) {
            u32x4 vals[SB];
#pragma unroll
            for (int u = 0; u < SB; ++u) {
                const int e = e0 + 64 * u;
                vals[u] = zero4;
                if (e < nxv) {
                    const int pi = e / CKV;
                    const int off = in_off[pi], c = c0 + (e - pi * CKV) * VEC;
                    if (off >= 0 && c < d.Cin) vals[u] = *(const u32x4*)(xb + off + c);
                }
            }
#pragma unroll
            for (int u = 0; u < SB; ++u) {
                const int e = e0 + 64 * u;
                if (e >= nxv) continue;
                const int pi = e / CKV;
                if (slope != 1.f) {
                    alignas(16) T tmp[VEC];
                    *(u32x4*)tmp = vals[u];
#pragma unroll
                    for (int q = 0; q < VEC; ++q) {
                        float f = Elt<T>::ld(&tmp[q]);
                        f = f > 0.f ? f : f * slope;
                        Elt<T>::st(&tmp[q], f);
                    }
                    vals[u] = *(const u32x4*)tmp;
                }
                *(u32x4*)(xt + (size_t)pi * XS + (e - pi * CKV) * VEC) = vals[u];
            }
        }
        for (int e0 = lane; e0 < nwv; e0 += 64 * SB) {
            u32x4 vals[SB];
#pragma unroll
            for (int u = 0; u < SB; ++u) {
                const int e = e0 + 64 * u;
                vals[u] = zero4;
                if (e < nwv) {
                    const int row = e / CKV;
                    const int t = row / BN, co = co0 + (row - t * BN), c = c0 + (e - row * CKV) * VEC;
                    if (co < d.Cout && c < d.Cin) vals[u] = *(const u32x4*)(wg + ((size_t)tapw[t] * d.Cout + co) * d.Cin + c);
                }
            }
#pragma unroll
            for (int u = 0; u < SB; ++u) {
                const int e = e0 + 64 * u;
                if (e >= nwv) continue;
                const int row = e / CKV;
                *(u32x4*)(wt + (size_t)row * XS + (e - row * CKV) * VEC) = vals[u];
            }
        }
        wave_sync();                                            // this wave's tiles are complete
        for (int t = 0; t < d.ntaps; ++t) {
            const T* ap = xt + (size_t)(arow + (d.tap_dy[t] - G.dyMin) * IW + (d.tap_dx[t] - G.dxMin)) * XS;
            const T* bp = wt + (size_t)(t * BN + i) * XS;
#pragma unroll
            for (int ks = 0; ks < CK / 16; ++ks) mma_chunk16<NT>(ap + ks * 16, bp + ks * 16, 32 * XS, g, acc);
        }
        wave_sync();                                            // fragments consumed before the next chunk lands
    }
    // ---- the four partial tiles meet in LDS (each wave parks its own in its own region), then the usual epilogue
    float* pt = (float*)(regions + (size_t)w * region_bytes);   // [32][OS]
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) pt[((r & 3) + 8 * (r >> 2) + 4 * g) * OS + n * 32 + i] = acc[n][r];
    __syncthreads();
    const T* mask = (const T*)d.mask_src;
    const T* res = (const T*)d.res;
    const T* res2 = (const T*)d.res2;
    T* out = (T*)d.out;
    const size_t img = (size_t)b * d.Hout * d.Wout;
    const int fstride = region_bytes / (int)sizeof(float);
    const float* p0 = (const float*)regions;
    for (int e = tid; e < 32 * BNV; e += 256) {
        const int m = e / BNV, vcol = (e - m * BNV) * VEC;
        const int po = out_off[m], co = co0 + vcol;
        if (po < 0 || co >= d.Cout) continue;
        const size_t o = (img + po) * d.Cout + co;
        alignas(16) T mk[VEC], r1[VEC], r2[VEC], ov[VEC];
        if (mask) *(u32x4*)mk = *(const u32x4*)(mask + o);
        if (res) *(u32x4*)r1 = *(const u32x4*)(res + o);
        if (res2) *(u32x4*)r2 = *(const u32x4*)(res2 + o);
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
            const int idx = m * OS + vcol + q;
            float x = ((p0[idx] + p0[fstride + idx]) + p0[2 * fstride + idx]) + p0[3 * fstride + idx];
            if (d.bias) x = x + d.bias[co + q];
            if (mask) x = x * (Elt<T>::ld(&mk[q]) > 0.f ? 1.f : d.mask_slope);
            if (res) x = x + Elt<T>::ld(&r1[q]);
            if (res2) x = Elt<T>::ld(&r2[q]) + x;
            if (d.out_div != 1.f) x = x / d.out_div;
            if (d.out_slope != 1.f) x = x > 0.f ? x : x * d.out_slope;
            Elt<T>::st(&ov[q], x);
        }
        *(u32x4*)(out + o) = *(const u32x4*)ov;
    }
}

// returns 1 when launched, 0 when the kernel does not apply
template <typename T, int NT, int CKM>
__global__ __launch_bounds__(256) void conv_gather_ks_kernel(msmc_conv_desc d, CvGeom G, int region_bytes) {
    cvks_body<T, NT, CKM>(d, G, region_bytes, blockIdx.x, blockIdx.y);
}
// the wave-split members of a grouped call on one grid (the phases of a transposed convolution, of a strided layer's data
// gradient: five to thirteen launches of tens of workgroups each otherwise)
struct CvKsGroupArgs {
    CvGroupArgs a;
    int reg[MSMC_GROUP_MAX];
};
template <typename T, int NT, int CKM>
__global__ __launch_bounds__(256) void conv_gather_ks_group_kernel(CvKsGroupArgs ga) {
    const int k = cv_group_member(ga.a.first, ga.a.n);
    const int id = blockIdx.x - ga.a.first[k];
    cvks_body<T, NT, CKM>(ga.a.d[k], ga.a.G[k], ga.reg[k], id % ga.a.nx[k], id / ga.a.nx[k]);
}

struct CvKsPlan {
    int applies, nt, ckm;
    CvGeom G;
    size_t reg, lds;
    unsigned gx, gy;
};
template <typename T>
static int cv_ks_plan(const msmc_conv_desc* d, CvKsPlan* pl) {
    constexpr int VEC = Elt<T>::VEC;
    pl->applies = 0;
    if ((d->Cin % VEC) != 0 || (d->Cout % VEC) != 0 || d->Cin < 8 * Elt<T>::CK) return 0;
    if ((long)d->Hin * d->Win * d->Cin >= (1L << 31) || (long)d->Hout * d->Wout >= (1L << 31)) return 0;
    size_t unused;
    int rc = cv_geometry(d, &pl->G, sizeof(T), 0, 0, &unused, 32);
    if (rc) return rc;
    const long npix = (long)pl->G.IH * pl->G.IW;
    const int nt = d->Cout > 32 ? 2 : 1;
    const size_t tables = (((size_t)(npix + 32 + 16) * sizeof(int)) + 15) & ~(size_t)15;
    auto region = [&](int ckm) {
        const size_t xs = (size_t)Elt<T>::CK * ckm + VEC;
        size_t r = ((size_t)npix + (size_t)d->ntaps * 32 * nt) * xs * sizeof(T);
        const size_t part = (size_t)32 * (32 * nt + 4) * sizeof(float);
        if (r < part) r = part;
        return (r + 15) & ~(size_t)15;
    };
    const int ckm = (tables + 4 * region(2) <= 150 * 1024) ? 2 : 1;
    pl->reg = region(ckm);
    pl->lds = tables + 4 * pl->reg;
    if (pl->lds > 160 * 1024) return 0;
    pl->nt = nt;
    pl->ckm = ckm;
    pl->gx = (unsigned)(pl->G.tilesX * pl->G.tilesY * d->B);
    pl->gy = (unsigned)((d->Cout + 32 * nt - 1) / (32 * nt));
    pl->applies = 1;
    return 0;
}
// SINGLE (d, G) or GROUP launch of one wave-split configuration
template <typename T>
static int cv_ks_dispatch(const CvKsPlan& pl, dim3 grid, size_t lds, msmc_stream stream, const msmc_conv_desc* d,
                          const CvKsGroupArgs* group) {
    int rc;
#define KS_GO(NT_, CKM_)                                                                                            \
    do {                                                                                                            \
        if (group) {                                                                                                \
            rc = msmc_allow_lds((const void*)conv_gather_ks_group_kernel<T, NT_, CKM_>, (int)lds);                  \
            if (rc) return rc;                                                                                      \
            MSMC_LAUNCH((conv_gather_ks_group_kernel<T, NT_, CKM_>), grid, dim3(256), lds, (msmc_stream_t)stream,   \
                        *group);                                                                                    \
        } else {                                                                                                    \
            rc = msmc_allow_lds((const void*)conv_gather_ks_kernel<T, NT_, CKM_>, (int)lds);                        \
            if (rc) return rc;                                                                                      \
            MSMC_LAUNCH((conv_gather_ks_kernel<T, NT_, CKM_>), grid, dim3(256), lds, (msmc_stream_t)stream, *d,     \
                        pl.G, (int)pl.reg);                                                                         \
        }                                                                                                           \
    } while (0)
    if (pl.nt == 2 && pl.ckm == 2) KS_GO(2, 2);
    else if (pl.nt == 2) KS_GO(2, 1);
    else if (pl.ckm == 2) KS_GO(1, 2);
    else KS_GO(1, 1);
#undef KS_GO
    msmc_conv_last = msmc_prof_name(msmc_kname(group ? "conv_gather_ks_group_kernel" : "conv_gather_ks_kernel", EltName<T>::v,
                                               pl.nt, pl.ckm));
    return msmc_check_launch();
}
template <typename T>
static int cv_ks_launch(const msmc_conv_desc* d, msmc_stream stream) {
    CvKsPlan pl;
    int rc = cv_ks_plan<T>(d, &pl);
    if (rc) return rc;
    if (!pl.applies) return 0;
    rc = cv_ks_dispatch<T>(pl, dim3(pl.gx, pl.gy), pl.lds, stream, d, nullptr);
    return rc ? rc : 1;
}
// variant-9 members of a grouped call (cv_family_group_launch): one grid per (column tiles, chunk width) configuration; a
// lone member of the call keeps the single launch of the per-member path
template <typename T>
struct CvKsFamily {
    typedef CvKsPlan Plan;
    typedef CvKsGroupArgs Args;
    static constexpr int min_members = 2;
    static constexpr bool lone_single = true;
    static bool mine(const msmc_conv_desc* d) { return d->variant == 9; }
    static int plan(const msmc_conv_desc* d, Plan* pl, int) { return cv_ks_plan<T>(d, pl); }
    static bool same(const Plan& p, const Plan& q) { return p.nt == q.nt && p.ckm == q.ckm; }
    static int blocks(const Plan& p) { return (int)(p.gx * p.gy); }
    static int* head(Args& ga, int m) { ga.a.n = m; return ga.a.first; }
    static void fill(Args& ga, int k, const msmc_conv_desc& d, const Plan& p) {
        ga.a.nx[k] = (int)p.gx;
        ga.a.d[k] = d;
        ga.a.G[k] = p.G;
        ga.reg[k] = (int)p.reg;
    }
    static int dispatch(const Plan& p, int blocks, size_t lds, msmc_stream stream, const msmc_conv_desc* d, const Args* group) {
        return cv_ks_dispatch<T>(p, group ? dim3((unsigned)blocks) : dim3(p.gx, p.gy), lds, stream, d, group);
    }
};

// which direct kernel would take this descriptor: 0 none, 1 small, 2 dot, 3 outer (mirrors cv_direct_launch)
static int cv_direct_kind(const msmc_conv_desc* d) {
    const int VEC = d->dtype == 0 ? 4 : 8;
    if (d->Cin <= 8 && d->Cout <= 16 && !(d->Cin == 1 && d->Cout % VEC == 0 && d->Cout >= 4 * VEC)) return 1;
    if (d->Cout == 1 && d->Cin % VEC == 0 && d->Cin >= 8 * VEC)
        return (size_t)d->ntaps * d->Cin * (d->dtype == 0 ? 4 : 2) <= 160 * 1024 ? 2 : 0;
    if (d->Cin == 1 && d->Cout % VEC == 0) return (size_t)d->ntaps * d->Cout * (d->dtype == 0 ? 4 : 2) <= 160 * 1024 ? 3 : 0;
    return 0;
}
static bool cv_takes_direct(const msmc_conv_desc* d) {
    return (d->variant == 8 || (d->variant == 0 && msmc_gather_generation >= 2)) && cv_direct_kind(d) != 0;
}

struct DirKey {
    int kind, ci, co;
};
static DirKey cv_direct_key(const msmc_conv_desc* d) {
    DirKey k = {cv_direct_kind(d), 0, 0};
    if (k.kind == 1) {
        k.ci = d->Cin <= 1 ? 1 : d->Cin <= 2 ? 2 : d->Cin <= 4 ? 4 : 8;
        k.co = d->Cout <= 1 ? 1 : d->Cout <= 4 ? 4 : d->Cout <= 8 ? 8 : 16;
    }
    return k;
}

// direct-kernel members with one key (same kernel instantiation) as one grid
template <typename T>
static int cv_direct_group_launch(const msmc_conv_desc* const* members, int m, DirKey key, msmc_stream stream) {
    constexpr int VEC = Elt<T>::VEC;
    DirGroupArgs a;
    a.n = m;
    int blocks = 0;
    size_t lds = 0;
    for (int k = 0; k < m; ++k) {
        const msmc_conv_desc* d = members[k];
        const long npoints = (long)d->B * d->QH * d->QW;
        long items = npoints, nb;
        size_t l;
        if (key.kind == 1) {
            nb = (npoints + 255) / 256;
            if (nb > 8L * MSMC_NUM_CU) nb = 8L * MSMC_NUM_CU;
            l = (size_t)d->ntaps * key.ci * key.co * sizeof(float);
        } else if (key.kind == 2) {
            nb = (npoints + 3) / 4;
            if (nb > 4L * MSMC_NUM_CU) nb = 4L * MSMC_NUM_CU;
            l = (size_t)d->ntaps * d->Cin * sizeof(T);
        } else {
            items = npoints * (d->Cout / VEC);
            nb = (items + 255) / 256;
            if (nb > 8L * MSMC_NUM_CU) nb = 8L * MSMC_NUM_CU;
            l = (size_t)d->ntaps * d->Cout * sizeof(T);
        }
        if (nb < 1) nb = 1;
        a.first[k] = blocks;
        a.items[k] = items;
        a.d[k] = *d;
        blocks += (int)nb;
        if (l > lds) lds = l;
    }
    a.first[m] = blocks;
    int rc;
    const dim3 grid((unsigned)blocks);
    if (key.kind == 1) {
#define DIRG_GO(CI_, CO_)                                                                                           \
    do {                                                                                                            \
        rc = msmc_allow_lds((const void*)conv_direct_small_group_kernel<T, CI_, CO_>, (int)lds);                    \
        if (rc) return rc;                                                                                          \
        MSMC_LAUNCH((conv_direct_small_group_kernel<T, CI_, CO_>), grid, dim3(256), lds, (msmc_stream_t)stream, a); \
    } while (0)
#define DIRG_CO(CI_)                                                                                                \
    do {                                                                                                            \
        if (key.co == 1) DIRG_GO(CI_, 1);                                                                           \
        else if (key.co == 4) DIRG_GO(CI_, 4);                                                                      \
        else if (key.co == 8) DIRG_GO(CI_, 8);                                                                      \
        else DIRG_GO(CI_, 16);                                                                                      \
    } while (0)
        if (key.ci == 1) DIRG_CO(1);
        else if (key.ci == 2) DIRG_CO(2);
        else if (key.ci == 4) DIRG_CO(4);
        else DIRG_CO(8);
#undef DIRG_CO
#undef DIRG_GO
        msmc_conv_last = msmc_prof_name(msmc_kname2("conv_direct_small_group_kernel", EltName<T>::v, key.ci, key.co, 0));
    } else if (key.kind == 2) {
        rc = msmc_allow_lds((const void*)conv_direct_dot_group_kernel<T>, (int)lds);
        if (rc) return rc;
        MSMC_LAUNCH((conv_direct_dot_group_kernel<T>), grid, dim3(256), lds, (msmc_stream_t)stream, a);
        msmc_conv_last = msmc_prof_name(msmc_kname("conv_direct_dot_group_kernel", EltName<T>::v, 0, -1));
    } else {
        rc = msmc_allow_lds((const void*)conv_direct_outer_group_kernel<T>, (int)lds);
        if (rc) return rc;
        MSMC_LAUNCH((conv_direct_outer_group_kernel<T>), grid, dim3(256), lds, (msmc_stream_t)stream, a);
        msmc_conv_last = msmc_prof_name(msmc_kname("conv_direct_outer_group_kernel", EltName<T>::v, 0, -1));
    }
    return msmc_check_launch();
}

extern "C" void msmc_conv_set_grouping(int on) { msmc_conv_grouping = on; }

template <typename T>
static int cv_group_launch(const msmc_conv_desc* descs, int n, msmc_stream stream) {
    Cv2Plan plans[MSMC_GROUP_LIMIT];
    bool pending[MSMC_GROUP_LIMIT], direct[MSMC_GROUP_LIMIT];
    bool done[MSMC_GROUP_LIMIT] = {};                           // members a family below has launched
    // third generation, persistent thin-layer members on one grid (off by default), fifth and seventh generation, thin-channel
    // members (variant 50), split-bf16 constant-matrix GEMMs (variants 36 / 37), wave-split members (variant 9)
    int rc = cv_family_group_launch<Cv3Family>(descs, n, stream, done);
    if (!rc) rc = cv4_group_launch(descs, n, stream, done);
    if (!rc) rc = cv_family_group_launch<Cv5Family>(descs, n, stream, done);
    if (!rc) rc = cv_family_group_launch<Cv7Family>(descs, n, stream, done);
    if (!rc) rc = cv_family_group_launch<Cv6Family>(descs, n, stream, done);
    if (!rc) rc = cv_family_group_launch<G1sFamily>(descs, n, stream, done);
    if (!rc) rc = cv_family_group_launch<CvKsFamily<T>>(descs, n, stream, done);
    if (rc) return rc;
    for (int i = 0; i < n; ++i) {
        pending[i] = direct[i] = false;
        const msmc_conv_desc* d = &descs[i];
        if (done[i]) continue;
        int nt_unused;
        const bool own_grid = d->variant == 9 || cv4_is_variant(d->variant) || g1_is_variant(d->variant);
        rc = (cv_takes_direct(d) || own_grid) ? 0 : cv2_plan<T>(d, &plans[i], &nt_unused);
        if (rc) return rc;
        if (own_grid) {                                         // (one launch each: they fill the chip on their own)
            rc = msmc_conv_gather(d, stream);
            if (rc) return rc;
        } else if (cv_takes_direct(d)) {
            direct[i] = true;
        } else if (!plans[i].applies) {                         // first-generation kernels: one launch each
            rc = msmc_conv_gather(d, stream);
            if (rc) return rc;
        } else {
            pending[i] = true;
        }
    }
    for (int i = 0; i < n; ++i) {                               // direct kernels: one grid per kernel instantiation
        if (!direct[i]) continue;
        const DirKey key = cv_direct_key(&descs[i]);
        const msmc_conv_desc* members[MSMC_GROUP_MAX];
        int m = 0;
        for (int j = i; j < n && m < MSMC_GROUP_MAX; ++j) {
            if (!direct[j]) continue;
            const DirKey kj = cv_direct_key(&descs[j]);
            if (kj.kind != key.kind || kj.ci != key.ci || kj.co != key.co) continue;
            members[m++] = &descs[j];
            direct[j] = false;
        }
        if (m == 1) {
            rc = msmc_conv_gather(members[0], stream);
        } else {
            ++msmc_conv_launches;
            rc = cv_direct_group_launch<T>(members, m, key, stream);
        }
        if (rc) return rc;
    }
    for (;;) {
        // leader = pending member with the largest grid; the others adopt its kernel parameters when they can
        int i = -1;
        for (int j = 0; j < n; ++j)
            if (pending[j] && (i < 0 || plans[j].gx * plans[j].gy > plans[i].gx * plans[i].gy)) i = j;
        if (i < 0) break;
        int members[MSMC_GROUP_MAX], m = 0;
        for (int jj = 0; jj < n && m < MSMC_GROUP_MAX; ++jj) {
            const int j = jj == 0 ? i : (jj <= i ? jj - 1 : jj);          // leader first, then the rest in order
            if (!pending[j]) continue;
            if (!Cv2Family<T>::same(plans[j], plans[i])) {
                Cv2Plan alt;
                rc = cv2_plan_forced<T>(&descs[j], &alt, plans[i].nt, plans[i].ckm, plans[i].sb);
                if (rc) return rc;
                if (!alt.applies) continue;
                plans[j] = alt;
            }
            members[m++] = j;
            pending[j] = false;
        }
        rc = cv_family_dispatch<Cv2Family<T>>(descs, plans, members, m, stream);
        if (rc) return rc;
    }
    return 0;
}

// n independent convolutions (msmc_conv_gather semantics each) issued as few launches as their kernel choices allow
extern "C" int msmc_conv_gather_group(const msmc_conv_desc* descs, int n, msmc_stream stream) {
    if (!descs || n <= 0 || n > MSMC_GROUP_LIMIT) return MSMC_E_SHAPE;
    bool same = true;
    for (int i = 0; i < n; ++i) {
        if (!cv_desc_ok(&descs[i])) return MSMC_E_SHAPE;
        same = same && descs[i].dtype == descs[0].dtype;
    }
    if (!msmc_conv_grouping || !same || n == 1) {
        for (int i = 0; i < n; ++i) {
            int rc = msmc_conv_gather(&descs[i], stream);
            if (rc) return rc;
        }
        return 0;
    }
    if (descs[0].dtype == 0) return cv_group_launch<float>(descs, n, stream);
    if (descs[0].dtype == 1) return cv_group_launch<unsigned short>(descs, n, stream);
    return MSMC_E_SHAPE;
}

