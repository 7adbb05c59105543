// vq_wide.inc -- nearest-centroid search for one wide head (k-means unit codebooks: d = 768 / 1024, any K) (included from vq.hip).
//
// The resident and streamed searches keep a wave's 16 frames in registers or LDS at full width and bring whole codeword rows
// to them: at d = 1024 neither the frame values nor two 16-row buffers fit.  This kernel is a GEMM with an arg-min epilogue
// instead, on the slice pipeline of wide_tile.inc (tiling, LDS buffers, hand-over, MFMA step and channel order: there).  A
// workgroup of four waves owns FT frames; the centroids pass by in tiles of KT.  WC of the four waves share a 16-frame tile and
// split the centroid tile between them (FT = 64 / WC, KT = 64 WC): few frames still give every CU several workgroups, at the
// price of WC times the centroid traffic from L2 -- the launcher picks WC from N.
//
// |x|^2 is summed from the frame fragments during the first centroid tile.  After a tile's last slice every lane compares its
// 16 distances (|x|^2 - 2 x.e_k) + |e_k|^2 in ascending k against its running (best, index): a later centroid wins only on a
// strictly smaller distance.  The norms of the rows past K in the last tile are +inf, so those columns cannot win whatever
// their rows hold.  After the last tile the four lane groups of a frame, then the WC waves (through LDS), are merged with the
// index as tie-break: the first minimum.  The winner's row then comes from embed_t in global memory (L2) and quant / diff are
// formed by the resident kernels' epilogue expression; the WC waves of a frame split the row's 16-byte pieces.
// Everything up to the merged (best, index) is vq_wide_argmin, which the labels-only kernel of vq_assign.inc calls as well.
// No atomics; every global store is a vector-memory store.  quant may alias x: a workgroup reads only its own frames' rows,
// and the last of those reads is behind a workgroup barrier before the first store.

// tests / tools (include/msmc_hip_debug.h): waves sharing a frame tile, 1 / 2 / 4; 0 = the launcher's choice
static int vq_wide_split = 0;
extern "C" void msmc_vq_wide_set_split(int wc) { vq_wide_split = wc; }

// The search itself, shared by vq_search_wide_kernel and vq_assign_wide_kernel (vq_assign.inc): the whole workgroup calls it
// and every lane (f, g) of the WC waves of a frame tile returns with the frame's first minimum (best, bi).  smem: the
// workgroup's dynamic LDS, of which it uses the first vqw_lds_bytes(WC) bytes; the callers' epilogues differ, the labels cannot.
template <int WC>
MSMC_DEV_INLINE void vq_wide_argmin(char* smem, const float* x, const float* __restrict__ embed_t,
                                    const float* __restrict__ enorm, int N, int d, int K, float& best, int& bi) {
    constexpr int WF = 4 / WC, FT = 16 * WF, KT = WIDE_KT * WC, ROWS = FT + KT;
    float* sl = (float*)smem;                                   // [2][ROWS][WIDE_PITCH]: frame rows, then centroid rows
    float* en = sl + 2 * ROWS * WIDE_PITCH;                     // [2][KT]
    float* mb = en + 2 * KT;                                    // [WC][FT] best distance of every wave
    int* mi = (int*)(mb + WC * FT);                             // [WC][FT] ... and its index
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int f = lane & 15, g = lane >> 4;
    const int wf = w / WC, wc = w - wf * WC;
    const int n0 = blockIdx.x * FT;
    const int nds = (d + WIDE_DS - 1) / WIDE_DS;
    const int nkt = (K + KT - 1) / KT;
    const int total = nkt * nds;
    const float inf = __builtin_inff();                         // the norm of a row past K: such a column can never win

    WideStage<FT, KT, 256> stage;
    stage.load(x, n0, N, embed_t, 0, K, d, 0, tid);
    stage.store(sl, d, 0, tid);
    wide_norm_store(en, 0, KT, tid, wide_norm_fetch(enorm, 0, KT, K, tid, inf));
    __syncthreads();

    int buf = 0;
    float xx = 0.f;
    best = inf;
    bi = 0;
    f32x4 acc[4];
    for (int q = 0; q < total; ++q) {
        const int kt = q / nds, s = q - kt * nds;
        const bool more = q + 1 < total;
        const bool next_tile = more && s + 1 == nds;
        const int kt1 = next_tile ? kt + 1 : kt, s1 = next_tile ? 0 : s + 1;      // slice q + 1
        float nn = 0.f;
        if (more) stage.load(x, n0, N, embed_t, kt1 * KT, K, d, s1 * WIDE_DS, tid);
        if (next_tile) nn = wide_norm_fetch(enorm, kt1, KT, K, tid, inf);
        if (s == 0) {
#pragma unroll
            for (int m = 0; m < 4; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        auto sumsq = [&](const f32x4& bv) {                     // |x|^2 from the frame fragments of the first centroid tile
            if (kt != 0) return;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                float sq = bv[jj] * bv[jj];
                xx = xx + sq;
            }
        };
        const float* slc = sl + buf * ROWS * WIDE_PITCH;
        wide_slice_mfma(slc + (wf * 16 + f) * WIDE_PITCH + 4 * g, slc + (FT + wc * WIDE_KT + f) * WIDE_PITCH + 4 * g,
                        wide_groups(d, s * WIDE_DS), acc, sumsq);
        if (more) stage.store(sl + (buf ^ 1) * ROWS * WIDE_PITCH, d, s1 * WIDE_DS, tid);
        if (next_tile) wide_norm_store(en, kt1, KT, tid, nn);

        if (s == nds - 1) {   // the tile's last slice: its 64 distances of this wave against the running minimum, ascending k
            if (kt == 0) xx = vq_group_sum(xx);
            const float* enc = wide_norm_tile(en, kt, KT) + wc * WIDE_KT + 4 * g;
            const int k0 = kt * KT + wc * WIDE_KT + 4 * g;
#pragma unroll
            for (int m = 0; m < 4; ++m) vq_take_min(acc[m], xx, enc + 16 * m, k0 + 16 * m, best, bi);
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
}

template <int WC>
__global__ __launch_bounds__(256) void vq_search_wide_kernel(const float* x, const float* __restrict__ embed_t,
                                                            const float* __restrict__ enorm, float* quant,
                                                            float* __restrict__ diff, int64_t* __restrict__ ind, int N, int d,
                                                            int K) {
    MSMC_DYN_LDS(smem);
    constexpr int WF = 4 / WC, FT = 16 * WF;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int f = lane & 15, g = lane >> 4;
    const int wf = w / WC, wc = w - wf * WC;
    const int n0 = blockIdx.x * FT;
    float best;
    int bi;
    vq_wide_argmin<WC>(smem, x, embed_t, enorm, N, d, K, best, bi);

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
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            f32x4 o4, s4;
            vq_st_piece(q4, x4, zero, true, o4, s4);
            *(f32x4*)(diff + (size_t)n * d + 4 * c4) = s4;
            *(f32x4*)(quant + (size_t)n * d + 4 * c4) = o4;
        }
    }
}

typedef void (*vq_search_wide_fn)(const float*, const float*, const float*, float*, float*, int64_t*, int, int, int);

static constexpr size_t vqw_lds_bytes(int wc) {
    return (wide_lds_floats(64 / wc, WIDE_KT * wc) + 2 * wc * (64 / wc)) * sizeof(float);
}

// waves per frame tile for N frames: the tests' switch, else the choice argued in vq_wide_launch (one place: the assignment of
// vq_assign.inc must run the instantiation the search would)
static inline int vq_wide_pick_split(int N) {
    const int wc = vq_wide_split;
    if (wc == 1 || wc == 2 || wc == 4) return wc;
    return N <= 32 * MSMC_NUM_CU ? 4 : ((N + 63) / 64 >= MSMC_NUM_CU ? 1 : 2);
}

static int vq_wide_launch(const float* x, const float* embed_t, const float* enorm, float* quant, float* diff, int64_t* ind,
                          int N, int d, int K, msmc_stream stream) {
    if (N < 0 || !wide_takes(d, K)) return MSMC_E_SHAPE;
    if ((double)N * d * 4.0 >= 4294967296.0) return MSMC_E_SHAPE;     // (as the other launchers: 32-bit frame byte offsets)
    if (N == 0) return 0;
    // Waves per frame tile.  A step (one 32-channel slice) is 32 MFMAs per wave behind a round trip to L2, so a CU wants
    // several workgroups to overlap; with few frames only the 16-frame workgroups (WC = 4) give it more than one.  Measured
    // on an MI355X (profiles/kmeans_vq.md; d = 1024, K = 1000): N = 6400: 867 / 450 / 318 us for WC = 1 / 2 / 4;
    // N = 2^17: 3.53 / 3.72 / 5.04 ms.  WC = 4 while all its workgroups are resident at once (two per CU: N <= 8192),
    // WC = 1 once the 64-frame workgroups fill every CU, WC = 2 in between (that range is not measured).
    const int wc = vq_wide_pick_split(N);
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
