// vq_wide.inc -- nearest-centroid search for one wide head (k-means unit codebooks: d = 768 / 1024, any K) (included from vq.hip).
//
// The resident and streamed searches keep a wave's 16 frames in registers or LDS at full width and bring whole codeword rows
// to them: at d = 1024 neither the frame values nor two 16-row buffers fit.  This kernel is a GEMM with an arg-min epilogue
// instead.  A workgroup of four waves owns FT frames; the centroids pass by in tiles of KT; the d axis is cut into slices of
// 32 channels, and one LDS buffer holds a slice of the FT frame rows followed by the same slice of the KT centroid rows, at a
// pitch of 36 floats.  Two such buffers: while the waves run the MFMA steps of slice q out of one, the rows of slice q + 1
// travel L2 -> registers (loads issued ahead of the MFMA steps) -> the other buffer (stores behind them); one workgroup
// barrier per slice closes the hand-over, as the chunk hand-over of vq_stream.inc does.
//
// A wave owns 16 frames x 64 centroids of the tile: four independent 16 x 16 accumulators on v_mfma_f32_16x16x4_f32 (exact
// fp32; four accumulators cover its 40-cycle dependent latency), channel order (slice, t, jj, g) -> 32 slice + 16 t + 4 g + jj.
// WC of the four waves share a 16-frame tile and split the centroid tile between them (FT = 64 / WC, KT = 64 WC): few frames
// still give every CU several workgroups, at the price of WC times the centroid traffic from L2 -- the launcher picks WC
// from N.
//
// |x|^2 is summed from the frame fragments during the first centroid tile.  After a tile's last slice every lane compares its
// 16 distances (|x|^2 - 2 x.e_k) + |e_k|^2 in ascending k against its running (best, index): a later centroid wins only on a
// strictly smaller distance.  The norms of the rows past K in the last tile are +inf, so those columns cannot win whatever
// their rows hold.  After the last tile the four lane groups of a frame, then the WC waves (through LDS), are merged with the
// index as tie-break: the first minimum.  The winner's row then comes from embed_t in global memory (L2) and quant / diff are
// formed by the resident kernels' epilogue expression; the WC waves of a frame split the row's 16-byte pieces.
// No atomics; every global store is a vector-memory store.  quant may alias x: a workgroup reads only its own frames' rows,
// and the last of those reads is behind a workgroup barrier before the first store.

#define VQW_DS 32                    // channels per slice
#define VQW_PITCH (VQW_DS + 4)       // floats per row of a slice buffer
#define VQW_MAX_D 2048

// tests / tools (include/msmc_hip_debug.h): waves sharing a frame tile, 1 / 2 / 4; 0 = the launcher's choice
static int vq_wide_split = 0;
extern "C" void msmc_vq_wide_set_split(int wc) { vq_wide_split = wc; }

template <int WC>
__global__ __launch_bounds__(256) void vq_search_wide_kernel(const float* x, const float* __restrict__ embed_t,
                                                            const float* __restrict__ enorm, float* quant,
                                                            float* __restrict__ diff, int64_t* __restrict__ ind, int N, int d,
                                                            int K) {
    MSMC_DYN_LDS(smem);
    constexpr int WF = 4 / WC, FT = 16 * WF, KT = 64 * WC, ROWS = FT + KT;
    constexpr int NST = (ROWS * (VQW_DS / 4) + 255) / 256;      // 16-byte pieces per work-item per slice
    float* sl = (float*)smem;                                   // [2][ROWS][VQW_PITCH]: frame rows, then centroid rows
    float* en = sl + 2 * ROWS * VQW_PITCH;                      // [2][KT]
    float* mb = en + 2 * KT;                                    // [WC][FT] best distance of every wave
    int* mi = (int*)(mb + WC * FT);                             // [WC][FT] ... and its index
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int f = lane & 15, g = lane >> 4;
    const int wf = w / WC, wc = w - wf * WC;
    const int n0 = blockIdx.x * FT;
    const int nds = (d + VQW_DS - 1) / VQW_DS;
    const int nkt = (K + KT - 1) / KT;
    const int total = nkt * nds;

    f32x4 st[NST];
    auto stage_load = [&](int q) {
        const int kt = q / nds, s0 = (q - kt * nds) * VQW_DS;
        const int sh = d - s0 < VQW_DS ? 2 : 3;                 // 16-byte pieces per row: 4 (the last slice of d % 32 == 16) or 8
#pragma unroll
        for (int i = 0; i < NST; ++i) {
            const int e = i * 256 + tid;
            const int r = e >> sh, c = s0 + 4 * (e & ((1 << sh) - 1));
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (r < FT) {
                if (n0 + r < N) v = *(const f32x4*)(x + (size_t)(n0 + r) * d + c);
            } else if (r < ROWS) {
                const int k = kt * KT + r - FT;
                if (k < K) v = *(const f32x4*)(embed_t + (size_t)k * d + c);
            }
            st[i] = v;
        }
    };
    auto stage_store = [&](int q, float* dst) {
        const int kt = q / nds, s0 = (q - kt * nds) * VQW_DS;
        const int sh = d - s0 < VQW_DS ? 2 : 3;
#pragma unroll
        for (int i = 0; i < NST; ++i) {
            const int e = i * 256 + tid;
            const int r = e >> sh, c4 = e & ((1 << sh) - 1);
            if (r < ROWS) *(f32x4*)(dst + r * VQW_PITCH + 4 * c4) = st[i];
        }
    };
    // the norms of centroid tile kt; rows past K: +inf, such a column can never win
    auto norm_of = [&](int kt) {
        const int k = kt * KT + tid;
        return (tid < KT && k < K) ? enorm[k] : __builtin_inff();
    };

    stage_load(0);
    stage_store(0, sl);
    if (tid < KT) en[tid] = norm_of(0);
    __syncthreads();

    int buf = 0;
    float xx = 0.f, best = __builtin_inff();
    int bi = 0;
    f32x4 acc[4];
    for (int q = 0; q < total; ++q) {
        const int kt = q / nds, s = q - kt * nds;
        const int nt = d - s * VQW_DS < VQW_DS ? 1 : 2;         // 16-channel groups of this slice
        const bool more = q + 1 < total;
        const bool next_tile = more && s + 1 == nds;
        float nn = 0.f;
        if (more) stage_load(q + 1);
        if (next_tile) nn = norm_of(kt + 1);
        if (s == 0) {
#pragma unroll
            for (int m = 0; m < 4; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const float* slc = sl + buf * ROWS * VQW_PITCH;
        const float* fb = slc + (wf * 16 + f) * VQW_PITCH + 4 * g;
        const float* cb = slc + (FT + wc * 64 + f) * VQW_PITCH + 4 * g;
        for (int t = 0; t < nt; ++t) {
            const f32x4 bv = *(const f32x4*)(fb + 16 * t);
            f32x4 av[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) av[m] = *(const f32x4*)(cb + m * 16 * VQW_PITCH + 16 * t);
            if (kt == 0) {
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    float sq = bv[jj] * bv[jj];
                    xx = xx + sq;
                }
            }
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                for (int m = 0; m < 4; ++m) acc[m] = mfma_f32_16x16x4(av[m][jj], bv[jj], acc[m]);
        }
        if (more) stage_store(q + 1, sl + (buf ^ 1) * ROWS * VQW_PITCH);
        if (next_tile && tid < KT) en[((kt + 1) & 1) * KT + tid] = nn;

        if (s == nds - 1) {   // the tile's last slice: its 64 distances of this wave against the running minimum, ascending k
            if (kt == 0) {
                xx = xx + wave_xor(xx, 16);
                xx = xx + wave_xor(xx, 32);
            }
            const float* enc = en + (kt & 1) * KT + wc * 64 + 4 * g;
            const int k0 = kt * KT + wc * 64 + 4 * g;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const f32x4 e4 = *(const f32x4*)(enc + 16 * m);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float t2 = 2.f * acc[m][r];
                    float dist = (xx - t2) + e4[r];
                    if (dist < best) { best = dist; bi = k0 + 16 * m + r; }
                }
            }
        }
        __syncthreads();         // slice q + 1 is complete, and nobody reads slice q (or this tile's norms) any more
        buf ^= 1;
    }

    // first minimum over the four lane groups of a frame, then over the WC waves that share it
    vq_merge_groups(best, bi);
    if constexpr (WC > 1) {
        if (g == 0) {
            mb[wc * FT + wf * 16 + f] = best;
            mi[wc * FT + wf * 16 + f] = bi;
        }
        __syncthreads();
        best = mb[wf * 16 + f];
        bi = mi[wf * 16 + f];
#pragma unroll
        for (int o = 1; o < WC; ++o) {
            float od = mb[o * FT + wf * 16 + f];
            int oi = mi[o * FT + wf * 16 + f];
            if (od < best || (od == best && oi < bi)) { best = od; bi = oi; }
        }
    }

    const int n = n0 + wf * 16 + f;
    if (n < N) {
        if (g == 0 && wc == 0) ind[n] = (int64_t)bi;
        const float* qrow = embed_t + (size_t)bi * d;               // winner row from global memory (L2)
        const float* xrow = x + (size_t)n * d;
        const int dv = d >> 2;
        // this lane owns the 16-byte pieces 4 wc + g, 4 (wc + WC) + g, ... of its frame
        for (int c4 = 4 * wc + g; c4 < dv; c4 += 4 * WC) {
            const f32x4 q4 = *(const f32x4*)(qrow + 4 * c4);
            const f32x4 x4 = *(const f32x4*)(xrow + 4 * c4);
            f32x4 o4, s4;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                float e = q4[jj] - x4[jj];
                o4[jj] = x4[jj] + e;
                s4[jj] = e * e;
            }
            *(f32x4*)(diff + (size_t)n * d + 4 * c4) = s4;
            *(f32x4*)(quant + (size_t)n * d + 4 * c4) = o4;
        }
    }
}

typedef void (*vq_search_wide_fn)(const float*, const float*, const float*, float*, float*, int64_t*, int, int, int);

static inline size_t vqw_lds_bytes(int wc) {
    const int ft = 64 / wc, kt = 64 * wc;
    return ((size_t)2 * (ft + kt) * VQW_PITCH + 2 * kt + 2 * wc * ft) * sizeof(float);
}

static int vq_wide_launch(const float* x, const float* embed_t, const float* enorm, float* quant, float* diff, int64_t* ind,
                          int N, int d, int K, msmc_stream stream) {
    if (N < 0 || d < 16 || d > VQW_MAX_D || d % 16 || K < 1) return MSMC_E_SHAPE;
    if ((double)N * d * 4.0 >= 4294967296.0) return MSMC_E_SHAPE;     // (as the other launchers: 32-bit frame byte offsets)
    if (N == 0) return 0;
    // Waves per frame tile.  A step (one 32-channel slice) is 32 MFMAs per wave behind a round trip to L2, so a CU wants
    // several workgroups to overlap; with few frames only the 16-frame workgroups (WC = 4) give it more than one.  Measured
    // on an MI355X (profiles/kmeans_vq.md; d = 1024, K = 1000): N = 6400: 867 / 450 / 318 us for WC = 1 / 2 / 4;
    // N = 2^17: 3.53 / 3.72 / 5.04 ms.  WC = 4 while all its workgroups are resident at once (two per CU: N <= 8192),
    // WC = 1 once the 64-frame workgroups fill every CU, WC = 2 in between (that range is not measured).
    int wc = vq_wide_split;
    if (wc != 1 && wc != 2 && wc != 4) wc = N <= 32 * MSMC_NUM_CU ? 4 : ((N + 63) / 64 >= MSMC_NUM_CU ? 1 : 2);
    vq_search_wide_fn fn = wc == 1 ? vq_search_wide_kernel<1> : wc == 2 ? vq_search_wide_kernel<2> : vq_search_wide_kernel<4>;
    const size_t lds = vqw_lds_bytes(wc);
    int rc = msmc_allow_lds((const void*)fn, (int)lds);
    if (rc) return rc;
    const int ft = 64 / wc;
    const int grid = (N + ft - 1) / ft;
    MSMC_LAUNCH(fn, dim3(grid), dim3(256), lds, (msmc_stream_t)stream, x, embed_t, enorm, quant, diff, ind, N, d, K);
    msmc_vq_last = msmc_prof_name("vq_search_wide_kernel");
    return msmc_check_launch();
}
