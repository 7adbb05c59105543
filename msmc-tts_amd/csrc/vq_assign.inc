// vq_assign.inc -- labels-only nearest-centroid assignment for one wide head: msmc_vq_assign_wide (included from vq.hip behind
// vq_wide.inc).  Unit extraction wants 8 bytes of label per frame, not the 2 d 4 bytes of quant / diff the search stores.
//
// The search IS the wide search's: vq_wide_argmin (vq_wide.inc) on the slice pipeline of wide_tile.inc -- same channel order,
// tiling, +inf norms past K and first-minimum merge -- in the instantiation (WC = 1 / 2 / 4 waves per frame tile) that
// vq_wide_pick_split gives msmc_vq_search_wide for the same N, msmc_vq_wide_set_split included.  ind is therefore what
// msmc_vq_search_wide writes, bit for bit.
//
// DISTANCE (dist != NULL; restated in numpy by tests/_unitscases.py, compared bit for bit).  dist[n] is the squared distance
// to the winner's row e = embed_t[ind[n]], recomputed as direct fp32 differences (the convention of kmeans_pp.hip: a frame that
// equals its centroid weighs exactly 0; the expanded form of the search can come out negative).  The 16-byte pieces
// c4 = 0 .. d / 4 - 1 of the row are dealt to 16 partial sums, piece c4 to partial c4 % 16:
//     partial[p] = (((+0 + s(p, 0)) + s(p, 1)) + ...)    over the pieces p, p + 16, p + 32, ... in ascending order, and within a
//                                                        piece its channels jj = 0 .. 3 in order, s = (x - e) * (x - e)
//     dist[n]    = (((+0 + partial[0]) + partial[1]) + ... + partial[15])
// Every difference, product and add is one rounding (-ffp-contract=off).  Partials no piece falls to (d < 256) are +0.  The
// order does not depend on the split: lane group g of wave wc owns the partials 4 wc + g + 4 WC j, j < 4 / WC, so that the
// WC waves of a frame share the row as the search's epilogue does; the 16 partials meet in LDS (over the slice buffers, which
// are free by then: the workgroup needs no more LDS than the search's) and lane group 0 of wave 0 adds them.  x and the
// winner's row come from L2 (the main loop has just read x).
// No atomics; every global store is a vector-memory store; quant and diff do not exist.

template <int WC>
__global__ __launch_bounds__(256) void vq_assign_wide_kernel(const float* __restrict__ x, const float* __restrict__ embed_t,
                                                            const float* __restrict__ enorm, int64_t* __restrict__ ind,
                                                            float* __restrict__ dist, int N, int d, int K) {
    MSMC_DYN_LDS(smem);
    constexpr int WF = 4 / WC, FT = 16 * WF, NP = 4 / WC;
    // [FT][16] partial sums of the frames' distances, over the slice buffers: nobody reads those behind the search's last
    // barrier, and a workgroup with LDS of its own for them would cost the 64-frame instantiation its fourth workgroup per CU
    static_assert((size_t)FT * 16 * sizeof(float) <= vqw_lds_bytes(WC), "the partial sums lie over the slice buffers");
    float* dp = (float*)smem;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int f = lane & 15, g = lane >> 4;
    const int wf = w / WC, wc = w - wf * WC;
    const int n0 = blockIdx.x * FT;
    float best;
    int bi;
    vq_wide_argmin<WC>(smem, x, embed_t, enorm, N, d, K, best, bi);

    const int n = n0 + wf * 16 + f;
    if (n < N && g == 0 && wc == 0) ind[n] = (int64_t)bi;
    if (dist == nullptr) return;                                // (the same for the whole grid)

    float part[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) part[j] = 0.f;
    if (n < N) {
        const float* qrow = embed_t + (size_t)bi * d;
        const float* xrow = x + (size_t)n * d;
        const int dv = d >> 2;
        for (int c0 = 0; c0 < dv; c0 += 16) {
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                const int c4 = c0 + 4 * WC * j + 4 * wc + g;
                if (c4 < dv) {
                    const f32x4 q4 = *(const f32x4*)(qrow + 4 * c4);
                    const f32x4 x4 = *(const f32x4*)(xrow + 4 * c4);
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        float df = x4[jj] - q4[jj];
                        float sq = df * df;
                        part[j] = part[j] + sq;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NP; ++j) dp[(wf * 16 + f) * 16 + 4 * WC * j + 4 * wc + g] = part[j];
    __syncthreads();
    if (n < N && g == 0 && wc == 0) {
        float s = 0.f;
#pragma unroll
        for (int p4 = 0; p4 < 4; ++p4) {
            const f32x4 v = *(const f32x4*)(dp + (wf * 16 + f) * 16 + 4 * p4);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) s = s + v[jj];
        }
        dist[n] = s;
    }
}

typedef void (*vq_assign_wide_fn)(const float*, const float*, const float*, int64_t*, float*, int, int, int);

static int vq_assign_launch(const float* x, const float* embed_t, const float* enorm, int64_t* ind, float* dist, int N, int d,
                            int K, msmc_stream stream) {
    if (N < 0 || !wide_takes(d, K)) return MSMC_E_SHAPE;
    if ((double)N * d * 4.0 >= 4294967296.0) return MSMC_E_SHAPE;     // (32-bit frame byte offsets, as the search)
    if ((((uintptr_t)x | (uintptr_t)embed_t) & 15) != 0) return MSMC_E_SHAPE;
    if (N == 0) return 0;
    const int wc = vq_wide_pick_split(N);
    vq_assign_wide_fn fn = wc == 1 ? vq_assign_wide_kernel<1> : wc == 2 ? vq_assign_wide_kernel<2> : vq_assign_wide_kernel<4>;
    const int ft = 64 / wc;
    const size_t lds = vqw_lds_bytes(wc);
    int rc = msmc_allow_lds((const void*)fn, (int)lds);
    if (rc) return rc;
    const int grid = (N + ft - 1) / ft;
    MSMC_LAUNCH(fn, dim3(grid), dim3(256), lds, (msmc_stream_t)stream, x, embed_t, enorm, ind, dist, N, d, K);
    msmc_vq_last = msmc_prof_name("vq_assign_wide_kernel");
    return msmc_check_launch();
}
