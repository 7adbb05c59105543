// gemm1.inc -- 1-tap (kernel-size-1, unit-stride) layers as a plain channel GEMM on the matrix cores (variant 34, bf16
// and exact fp32).
// Included by conv.hip; entered through msmc_conv_gather like every other forward / data-gradient kernel.
//
// Replaces, for the layers it takes, the gather machinery (lattice / tap tables, halo tiles) that makes the general kernels
// spend 9-17 us on 1-2 GFLOP: the Q/K/V and output projections of the FFT blocks (reference acoustic_models/transformer.py:
// 296-315), the quantiser's 1x1 pre- / post-processor stacks and `in_linear` / `mel_predictor` (vqgantts/msmc_vqgan.py:
// 115-136, 287-300), the prior predictor's res/skip and projection layers (modules.py:229-251) -- and all their data
// gradients (the bank keeps the transposed slice, so those are the same GEMM).
//
//   out[m][n] = epilogue( sum_k act(x[m][k]) * w[n][k] + bias[n] ),  m over B*H*W pixels, both operands k-contiguous
//
// Workgroup = 128 pixels x 128 channels, sixteen waves of 32 x 32 (one accumulator of v_mfma_f32_32x32x16_bf16 each: four
// waves per SIMD hide each other's LDS and epilogue latency; four and eight waves measured 17-24 and 10-17 us).  The
// contraction runs in 64-channel chunks, up to four of them in flight at once in LDS stages filled by LDS-DMA
// (global_load_lds_dwordx4: no staging registers; 16 KB of x rows + 16 KB of w rows per stage; out-of-range rows / channels
// read a zero chunk: at K <= 256 the whole contraction is requested before the first wait); rows are 128
// bytes with the 16-byte pieces XOR-ed by (row >> 1) & 7 AT THE SOURCE, which makes every ds_read_b128 of a fragment
// bank-conflict-free.  Operand roles are swapped (A = weight rows, B = pixel rows), so a lane's accumulator registers are
// four runs of four consecutive channels of ONE pixel: bias / mask / residuals / leaky-ReLU / bf16 pack in registers,
// 8-byte stores, no LDS round trip in the epilogue.  Workgroups that share a pixel tile are numbered so that they land on
// the same XCD (its L2 serves the re-read).
#define G1_TN 128
#define G1_STAGES 4

struct Gemm1Params {
    int M, tilesM, tilesN, nchunks;
    int by_channel;          // blocks of one CHANNEL tile share an XCD (weights larger than the activations), else of one pixel tile
};

__device__ const u32x4 g1_zero_chunk = {0u, 0u, 0u, 0u};

// T = unsigned short (bf16 storage) or float.  A chunk is 128 bytes of every row in both cases (64 bf16 / 32 fp32
// channels), so operand movement, LDS image and swizzle are the same code; the fp32 form multiplies exactly on
// v_mfma_f32_32x32x2_f32 (a lane's 16-byte piece holds four k values of its row: MFMA step e of a piece pair takes element e
// of the pieces 2j and 2j + 1 -- any pairing of k values is a valid order of the sum as long as both operands use it) and
// writes fp32: the framed-DFT / mel-basis GEMMs of the spectral front-ends (csrc/spectral.hip; reference utils/audio.py:
// 398-419, stft_loss.py:76-108), which the general wave-split kernel ran at 14 % of the fp32 matrix-core peak.
// MW = waves along the pixel axis (4: 128 x 128 tile, sixteen waves -- variant 34; 2: 64 x 128 tile, eight waves -- variant
// 35, for the GEMMs with a few hundred pixel rows, where the larger tile leaves most CUs without a workgroup).
template <typename T, int MW>
__global__ __launch_bounds__(256 * MW) void conv_gemm1_kernel(msmc_conv_desc d, Gemm1Params P) {
    MSMC_DYN_LDS(smem);
    constexpr int TM = 32 * MW, XP = TM / 8, NP = XP + G1_TN / 8, PPW = NP / (4 * MW);   // pieces: x rows, all, per wave
    static_assert(NP % (4 * MW) == 0, "every wave issues the same number of LDS-DMA instructions");
    constexpr bool F32 = sizeof(T) == 4;
    constexpr int KC = 128 / (int)sizeof(T), PE = 16 / (int)sizeof(T);      // channels per chunk / per 16-byte piece
    const int tid = threadIdx.x, w = wave_uniform(tid >> 6), lane = tid & 63, li = lane & 31, g = lane >> 5;
    // block -> (pixel tile, channel tile): the channel tiles of a pixel tile run on one XCD (blocks go round-robin over 8)
    // (each XCD has its own L2: the operand that is re-read by the tiles along the other axis should be the one that fits
    //  it -- the framed-DFT basis of 10 MB against 3 MB of frames is streamed once per XCD slice instead of once per XCD)
    int tm, tn;
    if (!P.by_channel) {
        const int b = blockIdx.x, per = 8 * P.tilesN;
        const int grp = b / per, r = b - grp * per;
        tm = grp * 8 + (r & 7);
        tn = r >> 3;
        if (tm >= P.tilesM) return;                       // (padding blocks of the last group)
    } else {
        const int b = blockIdx.x, per = 8 * P.tilesM;
        const int grp = b / per, r = b - grp * per;
        tn = grp * 8 + (r & 7);
        tm = r >> 3;
        if (tn >= P.tilesN) return;
    }
    const int m0 = tm * TM, n0 = tn * G1_TN;
    const int wm = (w % MW) * 32, wn = (w / MW) * 32;     // this wave's 32 pixels x 32 channels of the tile
    const T* xg = (const T*)d.x;
    const T* wg = (const T*)d.w + (size_t)d.tap_w[0] * d.Cout * d.Cin;
    char* stage0 = smem;                                  // stage s: [TM x rows][128 B] then [128 w rows][128 B]
    const int STAGE = (TM + G1_TN) * 128;

    // ---- LDS-DMA of chunk c into stage s: NP pieces of 1 KiB (8 rows each), PPW per wave
    auto request = [&](int c, int s) {
        char* st = stage0 + (size_t)s * STAGE;
        const int k0 = c * KC;
#pragma unroll
        for (int q = 0; q < PPW; ++q) {
            const int piece = w * PPW + q;                // 0 .. XP-1: x rows, XP .. NP-1: w rows
            const int row = (piece < XP ? piece : piece - XP) * 8 + (lane >> 3);
            const int kk = k0 + (((lane & 7) ^ ((row >> 1) & 7)) * PE);      // logical 16-byte piece of the row -> channels
            const T* src;
            if (piece < XP) {
                const int m = m0 + row;
                src = (m < P.M && kk < d.Cin) ? xg + (size_t)m * d.Cin + kk : (const T*)&g1_zero_chunk;
            } else {
                const int n = n0 + row;
                src = (n < d.Cout && kk < d.Cin) ? wg + (size_t)n * d.Cin + kk : (const T*)&g1_zero_chunk;
            }
            lds_dma16(src, st + (size_t)piece * 1024);
        }
    };

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float slope = d.in_slope;
    const int xrow = wm + li, wrow = wn + li;
    const int xkey = (xrow >> 1) & 7, wkey = (wrow >> 1) & 7;

    auto compute = [&](int slot) {
        const char* xs = stage0 + (size_t)slot * STAGE;
        const char* ws = xs + TM * 128;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            u32x4 xf = *(const u32x4*)(xs + (size_t)xrow * 128 + (((2 * ks + g) ^ xkey) << 4));
            const u32x4 wf = *(const u32x4*)(ws + (size_t)wrow * 128 + (((2 * ks + g) ^ wkey) << 4));
            if (F32) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float xv = __uint_as_float(xf[e]);
                    if (slope != 1.f) xv = fmaxf(xv, xv * slope);
                    acc = mfma_f32_32x32x2(__uint_as_float(wf[e]), xv, acc);
                }
            } else {
                if (slope != 1.f) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) xf[q] = bf16x2_leaky(xf[q], slope);
                }
                acc = mfma_bf16_32x32x16(__builtin_bit_cast(bf16x8, wf), __builtin_bit_cast(bf16x8, xf), acc);
            }
        }
    };
    if (P.nchunks <= G1_STAGES) {
        // the whole contraction fits the stages: ALL pieces are requested before the first wait (one memory latency)
        for (int c = 0; c < P.nchunks; ++c) request(c, c);
        lds_dma_wait();                                   // this wave's pieces ...
        __syncthreads();                                  // ... everyone's
        for (int c = 0; c < P.nchunks; ++c) compute(c);
    } else {
        // deeper contractions (the fp32 DFT GEMMs: 15-65 chunks): a ring -- chunks c+1 .. c+3 in flight under the MFMAs
        // of chunk c, one LDS-only barrier per chunk, counted waits (every wave issues PPW pieces per chunk; chunks past
        // the end repeat the last one into a free slot, so the count is a constant)
        const int last = P.nchunks - 1;
#pragma unroll
        for (int c = 0; c < G1_STAGES - 1; ++c) request(c, c);
        int slot = 0, islot = G1_STAGES - 1;
        for (int c = 0; c < P.nchunks; ++c) {
            lds_dma_wait_n<(G1_STAGES - 2) * PPW>();
            block_sync_lds();                             // chunk c landed for everyone; the slot of chunk c-1 is free
            const int nx = c + G1_STAGES - 1;
            request(nx < last ? nx : last, islot);
            if (++islot == G1_STAGES) islot = 0;
            compute(slot);
            if (++slot == G1_STAGES) slot = 0;
        }
        lds_dma_wait();
    }

    // ---- epilogue in registers: lane (li, g) owns pixel wm + li and channels wn + 8 q + 4 g + (0..3)
    const T* mask = (const T*)d.mask_src;
    const T* res = (const T*)d.res;
    const T* res2 = (const T*)d.res2;
    T* out = (T*)d.out;
    const float mslope = d.mask_slope, odiv = d.out_div, oslope = d.out_slope;
    const int m = m0 + wm + li;
    if (m >= P.M) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int n = n0 + wn + 8 * q + 4 * g;
        if (n >= d.Cout) continue;                        // (Cout % 4 == 0: a run is all in or all out)
        const size_t o = (size_t)m * d.Cout + n;
        f32x4 bv = {0.f, 0.f, 0.f, 0.f};
        if (d.bias) bv = *(const f32x4*)(d.bias + n);
        float mk[4] = {0.f, 0.f, 0.f, 0.f}, r1[4] = {0.f, 0.f, 0.f, 0.f}, r2[4] = {0.f, 0.f, 0.f, 0.f};
        if (F32) {
            if (mask) { const f32x4 t = *(const f32x4*)(mask + o); for (int j = 0; j < 4; ++j) mk[j] = t[j]; }
            if (res) { const f32x4 t = *(const f32x4*)(res + o); for (int j = 0; j < 4; ++j) r1[j] = t[j]; }
            if (res2) { const f32x4 t = *(const f32x4*)(res2 + o); for (int j = 0; j < 4; ++j) r2[j] = t[j]; }
        } else {
            u32x2 t;
            if (mask) { t = *(const u32x2*)(mask + o); for (int j = 0; j < 4; ++j) mk[j] = bf16_bits_to_f32((unsigned short)(t[j >> 1] >> (16 * (j & 1)))); }
            if (res) { t = *(const u32x2*)(res + o); for (int j = 0; j < 4; ++j) r1[j] = bf16_bits_to_f32((unsigned short)(t[j >> 1] >> (16 * (j & 1)))); }
            if (res2) { t = *(const u32x2*)(res2 + o); for (int j = 0; j < 4; ++j) r2[j] = bf16_bits_to_f32((unsigned short)(t[j >> 1] >> (16 * (j & 1)))); }
        }
        float ov[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) ov[j] = acc[4 * q + j] + bv[j];
        if (mask) {
#pragma unroll
            for (int j = 0; j < 4; ++j) ov[j] = ov[j] * (mk[j] > 0.f ? 1.f : mslope);
        }
        if (res) {
#pragma unroll
            for (int j = 0; j < 4; ++j) ov[j] = ov[j] + r1[j];
        }
        if (res2) {
#pragma unroll
            for (int j = 0; j < 4; ++j) ov[j] = r2[j] + ov[j];
        }
        if (odiv != 1.f) {                                  // (bf16 output: the reciprocal -- the IEEE division is 11 instructions per value)
            const float rdiv = 1.f / odiv;
#pragma unroll
            for (int j = 0; j < 4; ++j) ov[j] = F32 ? ov[j] / odiv : ov[j] * rdiv;
        }
        if (oslope != 1.f) {
#pragma unroll
            for (int j = 0; j < 4; ++j) ov[j] = ov[j] > 0.f ? ov[j] : ov[j] * oslope;
        }
        if (F32) {
            const f32x4 pk = {ov[0], ov[1], ov[2], ov[3]};
            *(f32x4*)(out + o) = pk;
        } else {
            const u32x2 pk = {pack_bf16x2(ov[0], ov[1]), pack_bf16x2(ov[2], ov[3])};
            *(u32x2*)(out + o) = pk;
        }
    }
}

// ---- split-bf16 form for the CONSTANT-matrix GEMMs of the spectral front-ends (variants 36 / 37) ---------------------------
// The framed-DFT and mel / filter-bank projections (reference utils/audio.py:398-419, stft_loss.py:76-108) multiply fp32
// data by a matrix that never changes.  v_mfma_f32_32x32x2_f32 prices them at 157 TFLOP/s and their small grids (100-170
// workgroups of 15-65 chunks) spend 60 % of their time in it.  Here the matrix arrives PRE-SPLIT -- per row and 32-value
// chunk [hi(32 bf16) | lo(32 bf16)], hi = bf16(w), lo = bf16(w - hi): the same 128 bytes a chunk of the fp32 row takes, so
// staging, LDS image and swizzle are the fp32 form's -- and the data operand is split in registers after its fragment read
// (two packed conversions and two subtractions per value pair); three products  w_hi x_hi + w_lo x_hi + w_hi x_lo  on
// v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  Dropped: w_lo x_lo (2^-18 relative) and the residuals of the two-piece
// splits (2^-18 each): ~2^-16 of |w||x| per product -- used by the bf16 training configuration only (the fp32 parity
// configuration keeps the exact fp32 form), inside the 1e-4 bar of the spectral fixtures at their scales.
// x fp32 [M][Cin] (Cin % 4 == 0), w image [Cout][nchunks][64] bf16, out fp32 [M][Cout]; no epilogue operands.
template <int MW>
MSMC_DEV void g1s_body(const msmc_conv_desc& d, const Gemm1Params& P, const int bid) {
    MSMC_DYN_LDS(smem);
    constexpr int TM = 32 * MW, XP = TM / 8, NP = XP + G1_TN / 8, PPW = NP / (4 * MW);
    static_assert(NP % (4 * MW) == 0, "every wave issues the same number of LDS-DMA instructions");
    const int tid = threadIdx.x, w = wave_uniform(tid >> 6), lane = tid & 63, li = lane & 31, g = lane >> 5;
    int tm, tn;
    if (!P.by_channel) {
        const int b = bid, per = 8 * P.tilesN;
        const int grp = b / per, r = b - grp * per;
        tm = grp * 8 + (r & 7);
        tn = r >> 3;
        if (tm >= P.tilesM) return;
    } else {
        const int b = bid, per = 8 * P.tilesM;
        const int grp = b / per, r = b - grp * per;
        tn = grp * 8 + (r & 7);
        tm = r >> 3;
        if (tn >= P.tilesN) return;
    }
    const int m0 = tm * TM, n0 = tn * G1_TN;
    const int wm = (w % MW) * 32, wn = (w / MW) * 32;
    const float* xg = (const float*)d.x;
    const float* wg = (const float*)d.w;                  // (the split image, addressed in 4-byte units: 32 per chunk)
    const int ldw = P.nchunks * 32;
    char* stage0 = smem;
    const int STAGE = (TM + G1_TN) * 128;

    auto request = [&](int c, int s) {
        char* st = stage0 + (size_t)s * STAGE;
        const int k0 = c * 32;
#pragma unroll
        for (int q = 0; q < PPW; ++q) {
            const int piece = w * PPW + q;
            const int row = (piece < XP ? piece : piece - XP) * 8 + (lane >> 3);
            const int kk = k0 + (((lane & 7) ^ ((row >> 1) & 7)) * 4);
            const float* src;
            if (piece < XP) {
                const int m = m0 + row;
                src = (m < P.M && kk < d.Cin) ? xg + (size_t)m * d.Cin + kk : (const float*)&g1_zero_chunk;
            } else {
                const int n = n0 + row;
                src = n < d.Cout ? wg + (size_t)n * ldw + kk : (const float*)&g1_zero_chunk;
            }
            lds_dma16(src, st + (size_t)piece * 1024);
        }
    };

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int xrow = wm + li, wrow = wn + li;
    const int xkey = (xrow >> 1) & 7, wkey = (wrow >> 1) & 7;

    auto compute = [&](int slot) {
        const char* xs = stage0 + (size_t)slot * STAGE;
        const char* ws = xs + TM * 128;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            // the eight k values 16 ks + 8 g .. + 7 of this lane's rows: two fp32 pieces of x, one hi and one lo piece of w
            const u32x4 xa = *(const u32x4*)(xs + (size_t)xrow * 128 + (((4 * ks + 2 * g) ^ xkey) << 4));
            const u32x4 xb = *(const u32x4*)(xs + (size_t)xrow * 128 + (((4 * ks + 2 * g + 1) ^ xkey) << 4));
            const u32x4 wh = *(const u32x4*)(ws + (size_t)wrow * 128 + (((2 * ks + g) ^ wkey) << 4));
            const u32x4 wl = *(const u32x4*)(ws + (size_t)wrow * 128 + (((4 + 2 * ks + g) ^ wkey) << 4));
            u32x4 xh, xl;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float a = __uint_as_float(q < 2 ? xa[2 * q] : xb[2 * q - 4]);
                const float b = __uint_as_float(q < 2 ? xa[2 * q + 1] : xb[2 * q - 3]);
                const unsigned int hi = pack_bf16x2(a, b);
                xh[q] = hi;
                xl[q] = pack_bf16x2(a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xffff0000u));
            }
            acc = mfma_bf16_32x32x16(__builtin_bit_cast(bf16x8, wh), __builtin_bit_cast(bf16x8, xh), acc);
            acc = mfma_bf16_32x32x16(__builtin_bit_cast(bf16x8, wl), __builtin_bit_cast(bf16x8, xh), acc);
            acc = mfma_bf16_32x32x16(__builtin_bit_cast(bf16x8, wh), __builtin_bit_cast(bf16x8, xl), acc);
        }
    };
    if (P.nchunks <= G1_STAGES) {
        for (int c = 0; c < P.nchunks; ++c) request(c, c);
        lds_dma_wait();
        __syncthreads();
        for (int c = 0; c < P.nchunks; ++c) compute(c);
    } else {
        const int last = P.nchunks - 1;
#pragma unroll
        for (int c = 0; c < G1_STAGES - 1; ++c) request(c, c);
        int slot = 0, islot = G1_STAGES - 1;
        for (int c = 0; c < P.nchunks; ++c) {
            lds_dma_wait_n<(G1_STAGES - 2) * PPW>();
            block_sync_lds();
            const int nx = c + G1_STAGES - 1;
            request(nx < last ? nx : last, islot);
            if (++islot == G1_STAGES) islot = 0;
            compute(slot);
            if (++slot == G1_STAGES) slot = 0;
        }
        lds_dma_wait();
    }
    float* out = (float*)d.out;
    const int m = m0 + wm + li;
    if (m >= P.M) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int n = n0 + wn + 8 * q + 4 * g;
        if (n >= d.Cout) continue;
        const f32x4 pk = {acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
        *(f32x4*)(out + (size_t)m * d.Cout + n) = pk;
    }
}

template <int MW>
__global__ __launch_bounds__(256 * MW) void conv_gemm1s_kernel(msmc_conv_desc d, Gemm1Params P) {
    g1s_body<MW>(d, P, (int)blockIdx.x);
}
// Several split-bf16 constant-matrix GEMMs of one tile width as ONE grid (members of msmc_conv_gather_group with variants 36 /
// 37): the framed-DFT (or filter-bank) GEMMs of the five resolution front-ends are five grids of 20-170 workgroups each.
#define G1G_MAX 6
struct G1GroupArgs {
    int n;
    int first[G1G_MAX + 1];
    msmc_conv_desc d[G1G_MAX];
    Gemm1Params P[G1G_MAX];
};
static_assert(sizeof(G1GroupArgs) <= 4000, "kernel argument block");
template <int MW>
__global__ __launch_bounds__(256 * MW) void conv_gemm1s_group_kernel(G1GroupArgs a) {
    int k = 0;
    while (k + 1 < a.n && (int)blockIdx.x >= a.first[k + 1]) ++k;
    g1s_body<MW>(a.d[k], a.P[k], (int)blockIdx.x - a.first[k]);
}

static bool g1_is_variant(int variant) { return variant >= 34 && variant <= 37; }

// 1: launched, 0: the layer is outside this kernel's scope (the caller reports MSMC_E_SHAPE), < 0: error
static int g1_launch(const msmc_conv_desc* d, msmc_stream stream) {
    if ((d->dtype != 0 && d->dtype != 1) || d->ntaps != 1 || d->tap_dy[0] != 0 || d->tap_dx[0] != 0) return 0;
    if (d->QH != d->Hout || d->QW != d->Wout || d->Hout != d->Hin || d->Wout != d->Win) return 0;
    if (d->oy0 || d->ox0 || d->iy0 || d->ix0 || d->osy != 1 || d->osx != 1 || d->isy != 1 || d->isx != 1) return 0;
    const bool split = d->variant >= 36;        // fp32 data, pre-split constant matrix (conv_gemm1s_kernel): no epilogue operands
    if (split && (d->dtype != 0 || d->bias || d->res || d->res2 || d->mask_src || d->in_slope != 1.f || d->out_div != 1.f ||
                  d->out_slope != 1.f))
        return 0;
    const int pe = d->dtype == 0 ? 4 : 8, kc = d->dtype == 0 ? 32 : 64;     // channels per 16-byte piece / per chunk
    if (d->Cin % pe || d->Cout % 4 || d->Cin < 16) return 0;
    if (!(d->in_slope >= 0.f && d->in_slope <= 1.f)) return 0;
    if ((((size_t)d->x) | ((size_t)d->w) | ((size_t)d->out)) & 15) return 0;
    if ((((size_t)d->res) | ((size_t)d->res2) | ((size_t)d->mask_src)) & (d->dtype == 0 ? 15 : 7)) return 0;
    if (d->bias && (((size_t)d->bias) & 15)) return 0;
    const long M = (long)d->B * d->Hin * d->Win;
    if (M <= 0 || M > (1L << 30)) return 0;
    const int mw = (d->variant == 35 || d->variant == 37) ? 2 : 4, tm_ = 32 * mw;
    Gemm1Params P;
    P.M = (int)M;
    P.tilesM = (int)((M + tm_ - 1) / tm_);
    P.tilesN = (d->Cout + G1_TN - 1) / G1_TN;
    P.nchunks = (d->Cin + kc - 1) / kc;
    P.by_channel = (long)d->Cout > M && (long)d->Cout * d->Cin * (d->dtype == 0 ? 4 : 2) > (2L << 20);
    const int groups = P.by_channel ? (P.tilesN + 7) / 8 : (P.tilesM + 7) / 8;
    const int stages = P.nchunks < G1_STAGES ? P.nchunks : G1_STAGES;
    const size_t lds = (size_t)stages * (tm_ + G1_TN) * 128;
    const dim3 grid((unsigned)(groups * 8 * (P.by_channel ? P.tilesM : P.tilesN)));
#define G1_GO(T_, MW_, NAME_)                                                                                      \
    do {                                                                                                           \
        const int rc0 = msmc_allow_lds((const void*)conv_gemm1_kernel<T_, MW_>, (int)lds);                         \
        if (rc0) return rc0 < 0 ? rc0 : -rc0;                                                                      \
        MSMC_LAUNCH((conv_gemm1_kernel<T_, MW_>), grid, dim3(256 * MW_), lds, (msmc_stream_t)stream, *d, P);       \
        msmc_conv_last = msmc_prof_name(NAME_);                                                                    \
    } while (0)
#define G1S_GO(MW_, NAME_)                                                                                          \
    do {                                                                                                           \
        const int rc0 = msmc_allow_lds((const void*)conv_gemm1s_kernel<MW_>, (int)lds);                            \
        if (rc0) return rc0 < 0 ? rc0 : -rc0;                                                                      \
        MSMC_LAUNCH((conv_gemm1s_kernel<MW_>), grid, dim3(256 * MW_), lds, (msmc_stream_t)stream, *d, P);          \
        msmc_conv_last = msmc_prof_name(NAME_);                                                                    \
    } while (0)
    if (split && mw == 4) G1S_GO(4, "conv_gemm1s_kernel<4>");
    else if (split) G1S_GO(2, "conv_gemm1s_kernel<2>");
    else if (d->dtype == 0 && mw == 4) G1_GO(float, 4, "conv_gemm1_kernel<float, 4>");
    else if (d->dtype == 0) G1_GO(float, 2, "conv_gemm1_kernel<float, 2>");
    else if (mw == 4) G1_GO(unsigned short, 4, "conv_gemm1_kernel<unsigned short, 4>");
    else G1_GO(unsigned short, 2, "conv_gemm1_kernel<unsigned short, 2>");
#undef G1_GO
#undef G1S_GO
    return cv_launched(msmc_check_launch());
}


// plan of one split-form member (the checks of g1_launch)
struct G1sPlan { int applies; Gemm1Params P; int mw; unsigned blocks; size_t lds; };
static int g1s_plan(const msmc_conv_desc* d, G1sPlan* pl) {
    pl->applies = 0;
    if (d->dtype != 0 || d->ntaps != 1 || d->tap_dy[0] != 0 || d->tap_dx[0] != 0) return 0;
    if (d->QH != d->Hout || d->QW != d->Wout || d->Hout != d->Hin || d->Wout != d->Win) return 0;
    if (d->oy0 || d->ox0 || d->iy0 || d->ix0 || d->osy != 1 || d->osx != 1 || d->isy != 1 || d->isx != 1) return 0;
    if (d->bias || d->res || d->res2 || d->mask_src || d->in_slope != 1.f || d->out_div != 1.f || d->out_slope != 1.f) return 0;
    if (d->Cin % 4 || d->Cout % 4 || d->Cin < 16) return 0;
    if ((((size_t)d->x) | ((size_t)d->w) | ((size_t)d->out)) & 15) return 0;
    const long M = (long)d->B * d->Hin * d->Win;
    if (M <= 0 || M > (1L << 30)) return 0;
    pl->mw = d->variant == 37 ? 2 : 4;
    const int tm_ = 32 * pl->mw;
    Gemm1Params& P = pl->P;
    P.M = (int)M;
    P.tilesM = (int)((M + tm_ - 1) / tm_);
    P.tilesN = (d->Cout + G1_TN - 1) / G1_TN;
    P.nchunks = (d->Cin + 31) / 32;
    P.by_channel = (long)d->Cout > M && (long)d->Cout * d->Cin * 4 > (2L << 20);
    const int groups = P.by_channel ? (P.tilesN + 7) / 8 : (P.tilesM + 7) / 8;
    const int stages = P.nchunks < G1_STAGES ? P.nchunks : G1_STAGES;
    pl->lds = (size_t)stages * (tm_ + G1_TN) * 128;
    pl->blocks = (unsigned)(groups * 8 * (P.by_channel ? P.tilesM : P.tilesN));
    pl->applies = 1;
    return 0;
}
// split-form members of a grouped call (cv_family_group_launch): one grid per tile width; a member without company of its
// width keeps its own launch (g1_launch)
struct G1sFamily {
    typedef G1sPlan Plan;
    typedef G1GroupArgs Args;
    static_assert(G1G_MAX == MSMC_GROUP_MAX, "one bucket size for every family");
    static constexpr int min_members = 2;
    static constexpr bool lone_single = false;
    static bool mine(const msmc_conv_desc* d) { return d->variant == 36 || d->variant == 37; }
    static int plan(const msmc_conv_desc* d, Plan* pl, int) { return g1s_plan(d, pl); }
    static bool same(const Plan& p, const Plan& q) { return p.mw == q.mw; }
    static int blocks(const Plan& p) { return (int)p.blocks; }
    static int* head(Args& a, int m) { a.n = m; return a.first; }
    static void fill(Args& a, int k, const msmc_conv_desc& d, const Plan& p) {
        a.d[k] = d;
        a.P[k] = p.P;
    }
    static int dispatch(const Plan& p, int blocks, size_t lds, msmc_stream stream, const msmc_conv_desc*, const Args* group) {
        int rc;
        if (p.mw == 4) {
            rc = msmc_allow_lds((const void*)conv_gemm1s_group_kernel<4>, (int)lds);
            if (rc) return rc;
            MSMC_LAUNCH((conv_gemm1s_group_kernel<4>), dim3((unsigned)blocks), dim3(1024), lds, (msmc_stream_t)stream, *group);
            msmc_conv_last = msmc_prof_name("conv_gemm1s_group_kernel<4>");
        } else {
            rc = msmc_allow_lds((const void*)conv_gemm1s_group_kernel<2>, (int)lds);
            if (rc) return rc;
            MSMC_LAUNCH((conv_gemm1s_group_kernel<2>), dim3((unsigned)blocks), dim3(512), lds, (msmc_stream_t)stream, *group);
            msmc_conv_last = msmc_prof_name("conv_gemm1s_group_kernel<2>");
        }
        return msmc_check_launch();
    }
};
