// wide_tile.inc -- the slice pipeline of the wide single-head kernels, defined once (included from vq.hip ahead of vq_wide.inc
// and from losses.hip ahead of triple_wide.inc; no state and no exported symbol: it lives in two translation units).
//
// vq_search_wide_kernel and triple_loss_wide_kernel are the same GEMM with different epilogues: x.e_k of FT frame rows against
// the centroids, which pass by in tiles of KT rows (WIDE_KT per wave).  The d axis is cut into slices of WIDE_DS channels, and
// one LDS buffer holds a slice of the FT frame rows followed by the same slice of the KT centroid rows, at a pitch of
// WIDE_PITCH floats.  Two such buffers: while the waves run the MFMA steps of slice q out of one, the rows of slice q + 1 travel
// L2 -> registers (WideStage::load, issued ahead of the MFMA steps) -> the other buffer (WideStage::store, behind them); one
// workgroup barrier per slice closes the hand-over.  The norms of a centroid tile are double-buffered the same way, one tile
// ahead.  That loop -- `for q < total`, its barrier, and the epilogue behind a tile's last slice -- stays in each kernel.
//
// A wave's step: 16 frames x WIDE_KT centroids, four independent 16 x 16 accumulators on v_mfma_f32_16x16x4_f32 (exact fp32;
// four accumulators cover its 40-cycle dependent latency).  Lane (f, g) = (lane & 15, lane >> 4).  The order of the d-products
// of an accumulator element is (slice, t, jj, g) -> channel 32 slice + 16 t + 4 g + jj, and both kernels' tests rest on it.

#define WIDE_DS 32                   // channels per slice
#define WIDE_PITCH (WIDE_DS + 4)     // floats per row of a slice buffer
#define WIDE_KT 64                   // centroid rows of a tile per wave
#define WIDE_MAX_D 2048

// the shapes the wide kernels take: whole 16-channel groups, any number of centroids
static inline bool wide_takes(int d, int K) { return d >= 16 && d <= WIDE_MAX_D && d % 16 == 0 && K >= 1; }
// floats of LDS of the two slice buffers and the two norm tiles
static constexpr size_t wide_lds_floats(int ft, int kt) { return (size_t)2 * (ft + kt) * WIDE_PITCH + 2 * kt; }

// 16-channel groups of the slice that starts at channel s0: 2, or 1 for the last slice of d % 32 == 16
MSMC_DEV int wide_groups(int d, int s0) { return d - s0 < WIDE_DS ? 1 : 2; }
// ... and the shift that splits a piece number of that slice into (row, piece of the row): 8 pieces per row, or 4.
// (Its own select, not 1 + wide_groups: that form costs the kernels 40 - 100 instructions; profiles/wide_tile_refactor.md.)
MSMC_DEV int wide_piece_shift(int d, int s0) { return d - s0 < WIDE_DS ? 2 : 3; }

// one 16-byte piece of a row-major [rows][d] matrix; zeros past the last row or the window's end
MSMC_DEV f32x4 wide_piece(const float* __restrict__ m, int row, int rows, int d, int c, int cend) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row < rows && c < cend) v = *(const f32x4*)(m + (size_t)row * d + c);
    return v;
}

// One slice in flight between global memory and an LDS buffer, for a workgroup of NTHR work-items: its 16-byte pieces, row
// after row (FT frame rows, then KT centroid rows; 8 pieces per row, 4 in the short last slice), are dealt to the work-items
// in turn.
template <int FT, int KT, int NTHR>
struct WideStage {
    static constexpr int ROWS = FT + KT;
    static constexpr int NST = (ROWS * (WIDE_DS / 4) + NTHR - 1) / NTHR;     // pieces per work-item
    f32x4 st[NST];

    // channels s0 .. of the frames n0 .. n0 + FT - 1 of x [N][d] and of the centroids k0 .. k0 + KT - 1 of embed_t [K][d]
    MSMC_DEV_INLINE void load(const float* x, int n0, int N, const float* __restrict__ embed_t, int k0, int K, int d, int s0,
                              int tid) {
        const int sh = wide_piece_shift(d, s0);
#pragma unroll
        for (int i = 0; i < NST; ++i) {
            const int e = i * NTHR + tid;
            const int r = e >> sh, c = s0 + 4 * (e & ((1 << sh) - 1));
            st[i] = r < FT ? wide_piece(x, n0 + r, N, d, c, d) : wide_piece(embed_t, k0 + r - FT, r < ROWS ? K : 0, d, c, d);
        }
    }
    MSMC_DEV_INLINE void store(float* dst, int d, int s0, int tid) const {
        const int sh = wide_piece_shift(d, s0);
#pragma unroll
        for (int i = 0; i < NST; ++i) {
            const int e = i * NTHR + tid;
            const int r = e >> sh, c4 = e & ((1 << sh) - 1);
            if (r < ROWS) *(f32x4*)(dst + r * WIDE_PITCH + 4 * c4) = st[i];
        }
    }
};

// The MFMA steps of one slice.  fb / cb: this lane's frame row and its first centroid row in the slice buffer, at channel 4 g;
// nt = wide_groups.  on_frag sees every frame fragment between its read and its products (the search sums |x|^2 from it).
// (The loop is unrolled over its upper bound and leaves at t >= nt: written `t < nt` it is left rolled in this helper -- in the
//  kernels' own text it was unrolled -- and every group's LDS reads then wait in front of its MFMAs;
//  profiles/wide_tile_refactor.md.)
template <class OnFrag>
MSMC_DEV void wide_slice_mfma(const float* fb, const float* cb, int nt, f32x4 (&acc)[4], OnFrag on_frag) {
#pragma unroll
    for (int t = 0; t < WIDE_DS / 16; ++t) {
        if (t >= nt) break;
        const f32x4 bv = *(const f32x4*)(fb + 16 * t);
        f32x4 av[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) av[m] = *(const f32x4*)(cb + m * 16 * WIDE_PITCH + 16 * t);
        on_frag(bv);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
#pragma unroll
            for (int m = 0; m < 4; ++m) acc[m] = mfma_f32_16x16x4(av[m][jj], bv[jj], acc[m]);
    }
}

// The norms of centroid tile kt: work-item tid < KT fetches one (`fill` for a row past K) a tile ahead, and stores it into
// the tile's half of en [2][KT] behind the MFMA steps; wide_norm_tile is that half.
MSMC_DEV float wide_norm_fetch(const float* __restrict__ enorm, int kt, int KT, int K, int tid, float fill) {
    const int k = kt * KT + tid;
    return (tid < KT && k < K) ? enorm[k] : fill;
}
MSMC_DEV float* wide_norm_tile(float* en, int kt, int KT) { return en + (kt & 1) * KT; }
MSMC_DEV void wide_norm_store(float* en, int kt, int KT, int tid, float v) {
    if (tid < KT) wide_norm_tile(en, kt, KT)[tid] = v;
}
