// wgrad6.inc -- direct (vector ALU) bf16 weight gradient for THIN layers (desc.variant = 8; included by conv_wgrad.hip).
//
// The first layers of the resolution / period discriminators (reference msmctts/networks/hifigan/discriminator.py:15-154: DiscriminatorR /
// DiscriminatorP; spectrogram or waveform in, 1-16 channels) and their 1-channel output convolutions have weight
// gradients of 72-1536 numbers reduced over 10^5-10^6 pixels.  On the matrix-core kernels a 32 x 32 tile is >= 90 %
// padding there and the pixel axis goes through LDS staging: 65-270 us per call for 1-12 GFLOP.  Here one work-item owns
// one lattice point at a time and keeps a block of TPG taps x COB output channels x CIB input channels of dW in
// registers (<= 128 accumulators): per point one vector load of the output gradient, one of the input per tap, COB*CIB
// fused multiply-adds per tap.  Blocks of dW beyond that are further workgroups along y (they re-read the operands from
// L2).  End of the pixel range: wave sums by DPP, the four waves through LDS, ONE fp32 atomic per dW element and
// workgroup into the privatised copy (blockIdx.x mod dw_copies) -- the result contract of generations 1 / 2.
struct Wg6Params {
    int npoints, ppwg;            // lattice points of the whole batch, per workgroup
    int tgroups, nci, nco;        // blocks of dW along taps / input channels / output channels (grid y = their product)
    unsigned int m_qpi, m_qw;     // floor(2^32 / divisor) + 1 for the two divisions of a point index (wg6_div)
};

// n / dv for 0 <= n < 2^31 with m = floor(2^32 / dv) + 1: the estimate (n * m) >> 32 is the quotient or one above
// (error n * (m * dv - 2^32) / (dv * 2^32) < n / 2^32 * 1 <= 1/2 for n < 2^31); one correction step makes it exact
MSMC_DEV int wg6_div(int n, int dv, unsigned int m) {
    if (dv == 1) return n;                             // (m does not fit 32 bits)
    unsigned int q = __umulhi((unsigned int)n, m);
    if (q * (unsigned int)dv > (unsigned int)n) --q;
    return (int)q;
}

template <int N>
MSMC_DEV void wg6_load(const unsigned short* p, int valid, float (&v)[N]) {
    // `valid` leading elements exist (the rest read as zero); vector loads when the whole run exists and is aligned
    if (N >= 2 && valid >= N && (((size_t)p) & (N * 2 - 1 < 15 ? N * 2 - 1 : 15)) == 0) {
        if (N == 2) {
            const unsigned int w = *(const unsigned int*)p;
            v[0] = __uint_as_float(w << 16);
            v[1] = __uint_as_float(w & 0xffff0000u);
        } else if (N == 4) {
            const u32x2 w = *(const u32x2*)p;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                v[2 * j] = __uint_as_float(w[j] << 16);
                v[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
            }
        } else {
#pragma unroll
            for (int q = 0; q < N / 8; ++q) {
                const u32x4 w = *(const u32x4*)(p + 8 * q);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    v[8 * q + 2 * j] = __uint_as_float(w[j] << 16);
                    v[8 * q + 2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
                }
            }
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = j < valid ? bf16_bits_to_f32(p[j]) : 0.f;
}

template <int CIB, int COB, int TPG>
__global__ __launch_bounds__(256) void conv_wgrad6_kernel(msmc_conv_desc d, const unsigned short* __restrict__ gptr,
                                                         float* __restrict__ dw, float* __restrict__ db, Wg6Params P) {
    constexpr int NACC = TPG * COB * CIB;
    __shared__ float red[4][NACC + COB];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    int y = blockIdx.y;
    const int tg = y % P.tgroups;
    y /= P.tgroups;
    const int ci0 = (y % P.nci) * CIB, co0 = (y / P.nci) * COB, t0 = tg * TPG;
    const int nci_live = d.Cin - ci0 < CIB ? d.Cin - ci0 : CIB, nco_live = d.Cout - co0 < COB ? d.Cout - co0 : COB;
    if (d.dw_copies > 1) {                              // privatised accumulators: copy (workgroup index mod R)
        const int copy = blockIdx.x % d.dw_copies;
        dw += (size_t)copy * d.ntaps * d.Cout * d.Cin;
        if (db) db += (size_t)copy * d.Cout;
    }
    const bool do_bias = db != nullptr && tg == 0 && ci0 == 0;
    float acc[TPG][COB][CIB], bacc[COB];
#pragma unroll
    for (int tl = 0; tl < TPG; ++tl)
#pragma unroll
        for (int co = 0; co < COB; ++co)
#pragma unroll
            for (int ci = 0; ci < CIB; ++ci) acc[tl][co][ci] = 0.f;
#pragma unroll
    for (int co = 0; co < COB; ++co) bacc[co] = 0.f;
    const unsigned short* xg = (const unsigned short*)d.x;
    const float slope = d.in_slope;
    const int qpi = d.QH * d.QW;
    const int p0 = blockIdx.x * P.ppwg;
    const int p1 = p0 + P.ppwg < P.npoints ? p0 + P.ppwg : P.npoints;
    for (int p = p0 + tid; p < p1; p += 256) {
        const int b = wg6_div(p, qpi, P.m_qpi), q = p - b * qpi;
        const int qy = wg6_div(q, d.QW, P.m_qw), qx = q - qy * d.QW;
        float gv[COB];
        // (32-bit element offsets: wg6_launch refuses tensors of 2^31 elements or more)
        wg6_load<COB>(gptr + (size_t)(unsigned int)(((b * d.Hout + d.oy0 + qy * d.osy) * d.Wout + d.ox0 + qx * d.osx) * d.Cout + co0),
                      nco_live, gv);
        const int xrow0 = b * d.Hin;
        if (do_bias) {
#pragma unroll
            for (int co = 0; co < COB; ++co) bacc[co] = bacc[co] + gv[co];
        }
#pragma unroll
        for (int tl = 0; tl < TPG; ++tl) {
            const int t = t0 + tl;
            if (t >= d.ntaps) break;
            int iy = d.iy0 + qy * d.isy + d.tap_dy[t], ix = d.ix0 + qx * d.isx + d.tap_dx[t];
            bool inside = true;
            if (d.pad_mode == 1) {
                iy = reflect_index(iy, d.Hin);
                ix = reflect_index(ix, d.Win);
            } else {
                inside = (iy >= 0) && (iy < d.Hin) && (ix >= 0) && (ix < d.Win);
            }
            if (!inside) continue;
            float xv[CIB];
            wg6_load<CIB>(xg + (size_t)(unsigned int)(((xrow0 + iy) * d.Win + ix) * d.Cin + ci0), nci_live, xv);
            if (slope != 1.f) {
#pragma unroll
                for (int ci = 0; ci < CIB; ++ci) xv[ci] = xv[ci] > 0.f ? xv[ci] : xv[ci] * slope;
            }
#pragma unroll
            for (int co = 0; co < COB; ++co)
#pragma unroll
                for (int ci = 0; ci < CIB; ++ci) acc[tl][co][ci] = fmaf(gv[co], xv[ci], acc[tl][co][ci]);
        }
    }
    // wave sums (every lane ends with the total), four waves through LDS, one atomic per element and workgroup
#pragma unroll
    for (int tl = 0; tl < TPG; ++tl)
#pragma unroll
        for (int co = 0; co < COB; ++co)
#pragma unroll
            for (int ci = 0; ci < CIB; ++ci) {
                const float s = wave_sum(acc[tl][co][ci]);
                if (lane == 0) red[w][(tl * COB + co) * CIB + ci] = s;
            }
    if (do_bias) {
#pragma unroll
        for (int co = 0; co < COB; ++co) {
            const float s = wave_sum(bacc[co]);
            if (lane == 0) red[w][NACC + co] = s;
        }
    }
    __syncthreads();
    for (int e = tid; e < NACC + (do_bias ? COB : 0); e += 256) {
        const float s = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
        if (e >= NACC) {
            const int co = e - NACC;
            if (co < nco_live) atomicAdd(db + co0 + co, s);
            continue;
        }
        const int tl = e / (COB * CIB), r = e - tl * (COB * CIB);
        const int co = r / CIB, ci = r - co * CIB, t = t0 + tl;
        if (t < d.ntaps && co < nco_live && ci < nci_live)
            atomicAdd(dw + ((size_t)d.tap_w[t] * d.Cout + co0 + co) * d.Cin + ci0 + ci, s);
    }
}

// block shape for a layer: channel blocks that cover small channel counts exactly (CIB in {1,2,4,8,16}, COB in {1,4,8,16},
// CIB * COB <= 128) and as many taps per block as keep it within 128 accumulators (9 / 5 / 3 / 1)
#define WG6_TPG(CI_, CO_) (128 / ((CI_) * (CO_)) >= 9 ? 9 : 128 / ((CI_) * (CO_)) >= 5 ? 5 : 128 / ((CI_) * (CO_)) >= 3 ? 3 : 1)
static void wg6_shape(const msmc_conv_desc* d, int* cib, int* cob, int* tpg) {
    const int ci = d->Cin <= 1 ? 1 : d->Cin <= 2 ? 2 : d->Cin <= 4 ? 4 : d->Cin <= 8 ? 8 : 16;
    int co = d->Cout <= 1 ? 1 : d->Cout <= 4 ? 4 : d->Cout <= 8 ? 8 : 16;
    if (ci * co > 128) co = 8;
    *cib = ci; *cob = co; *tpg = WG6_TPG(ci, co);
}

// 0: launched; MSMC_E_SHAPE: outside the scope (bf16, few enough blocks of dW that re-reading the operands per block pays)
static int wg6_launch(const msmc_conv_desc* d, const void* g, float* dw, float* db, msmc_stream stream) {
    if (d->dtype != 1 || !(d->in_slope >= 0.f)) return MSMC_E_SHAPE;
    int cib, cob, tpg;
    wg6_shape(d, &cib, &cob, &tpg);
    Wg6Params P;
    P.tgroups = (d->ntaps + tpg - 1) / tpg;
    P.nci = (d->Cin + cib - 1) / cib;
    P.nco = (d->Cout + cob - 1) / cob;
    const long ny = (long)P.tgroups * P.nci * P.nco;
    if (ny > 96) return MSMC_E_SHAPE;                  // every block along y re-reads both operands: matrix-core territory
    const long npoints = (long)d->B * d->QH * d->QW;
    if (npoints <= 0 || npoints >= (1L << 31)) return MSMC_E_SHAPE;
    if ((long)d->B * d->Hin * d->Win * d->Cin >= (1L << 31) || (long)d->B * d->Hout * d->Wout * d->Cout >= (1L << 31)) return MSMC_E_SHAPE;
    P.npoints = (int)npoints;
    P.m_qpi = (unsigned int)((1ULL << 32) / (unsigned long long)(d->QH * (long)d->QW)) + 1u;
    P.m_qw = (unsigned int)((1ULL << 32) / (unsigned long long)d->QW) + 1u;
    // pixel split: enough workgroups to fill the chip (about four per CU over all y), at least 512 points each (the
    // closing reduction costs as much as a few hundred points)
    long nx = (4L * MSMC_NUM_CU + ny - 1) / ny;
    const long maxx = (npoints + 511) / 512;
    if (nx > maxx) nx = maxx;
    if (nx < 1) nx = 1;
    P.ppwg = (int)((npoints + nx - 1) / nx);
    nx = (npoints + P.ppwg - 1) / P.ppwg;
    const dim3 grid((unsigned)nx, (unsigned)ny);
#define WG6_GO(CI_, CO_)                                                                                           \
    MSMC_LAUNCH((conv_wgrad6_kernel<CI_, CO_, WG6_TPG(CI_, CO_)>), grid, dim3(256), 0, (msmc_stream_t)stream, *d,  \
                (const unsigned short*)g, dw, db, P)
#define WG6_CO(CI_)                                                                                                \
    do {                                                                                                           \
        if (cob == 1) WG6_GO(CI_, 1);                                                                              \
        else if (cob == 4) WG6_GO(CI_, 4);                                                                         \
        else if (cob == 8) WG6_GO(CI_, 8);                                                                         \
        else WG6_GO(CI_, (CI_ * 16 <= 128 ? 16 : 8));                                                              \
    } while (0)
    if (cib == 1) WG6_CO(1);
    else if (cib == 2) WG6_CO(2);
    else if (cib == 4) WG6_CO(4);
    else if (cib == 8) WG6_CO(8);
    else WG6_CO(16);
#undef WG6_CO
#undef WG6_GO
    static thread_local char name[64];
    snprintf(name, sizeof(name), "conv_wgrad6_kernel<%d, %d, %d>", cib, cob, tpg);
    msmc_conv_last = msmc_prof_name(name);
    return msmc_check_launch();
}
