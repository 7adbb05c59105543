// unit_embed.hip -- the decoder input of KMeansVQGANEmb from stored unit labels, for gfx950.  The codebook is frozen, so
// in_linear(embed_code(ind)) is a row of the projected table P = centers W^T + b [K][C]: the forward is a row gather (plus the
// utterance's global embedding), the backward a per-label sum of the incoming gradient.  Host side: msmctts_amd/hip/units.py
// (unit_embed); the table itself and its gradient's way back to in_linear are the framework's small GEMM.
//
// msmc_units_embed_fwd: out[b][t][:] = table[ind[b][t]][:] + glob[b][:] (one fp32 add; none without glob) where t < length[b] and
// 0 <= ind[b][t] < K, zeros in every other row.  The table is never read at an invalid label.  A memory-bound kernel: N C 4 bytes
// written, the table (K C 4 bytes, 2 MB at K = 2000, C = 256) served from L2.  One work-item per 16-byte piece: a workgroup of
// 256 takes UE_PIECES = 2048 consecutive pieces of the flattened [N][C / 4] output (32 KB: 32 rows at C = 256, at least 4 at
// C = 2048) in two passes of four pieces per work-item -- four labels, then four table rows and four glob rows in flight, then
// four stores; a wave stores 1 KB of consecutive bytes per instruction.  The grid is the number of such blocks of rows: 200 at
// N = 6400, 1600 at N = 51 200 with C = 256.  Beyond 8 per CU (2048 blocks, 64 MB of output) workgroups stride over the blocks:
// that bound only keeps the grid inside the launch limit for any B T C and is the usual one for streaming kernels; no size that
// reaches it has been timed against a one-block-per-workgroup grid (the tests run one: tests/_unitembedcases.py
// check_embed_forward_strided_grid).  Every element of out is written exactly once.
//
// msmc_units_embed_bwd: lab[n] = ind[n] where the row is valid (as above), else -1; ulab[n] = b where valid, else -1.  Then the
// launches of msmc_kmeans_stats (kmeans_stats.inc, shared as ema_wide.hip shares them) on (gout, lab) with K labels -> gtable and,
// with gglob, on (gout, ulab) with B labels -> gglob; both overwrite.  ORDER (restated in numpy by tests/_unitembedcases.py,
// compared bit for bit): per channel, the valid rows of label k (of utterance b) in ascending n are cut into runs of 64; a run
// partial is (((+0 + g[n_0]) + g[n_1]) + ...), the total (((+0 + partial_0) + partial_1) + ...) in ascending order.  No
// floating-point atomics: same inputs, same bits.
// Workspace: int64 lab [N], int64 ulab [N] (each rounded up to 16 bytes), max(K, B) floats of counts (rounded up to 16 bytes:
// the statistics pass writes them, nothing reads them), then the larger of the statistics workspaces for K and for B labels.
#include <msmc_rt.hpp>
#include <msmc_hip.h>

#include "kmeans_stats.inc"

#define UE_WG 256
#define UE_UNROLL 4
#define UE_PIECES 2048       // 16-byte pieces per block of rows: two passes of UE_WG x UE_UNROLL

__global__ __launch_bounds__(UE_WG) void ue_fwd_kernel(const int64_t* __restrict__ ind, const int64_t* __restrict__ length,
                                                      const float* __restrict__ table, const float* __restrict__ glob,
                                                      float* __restrict__ out, long pieces, long blocks, int T, int qpr, int K) {
    const int tid = threadIdx.x;
    for (long blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
        // the block's first piece: row n0 = utterance b0, frame t0, piece r0 of the row -- 64-bit divisions once per block (the
        // same in every work-item), 32-bit ones per piece: a piece is fewer than UE_PIECES + qpr pieces behind n0's first
        const long p0 = blk * UE_PIECES;
        const long n0 = p0 / qpr, b0 = n0 / T;
        const unsigned r0 = (unsigned)(p0 - n0 * qpr), t0 = (unsigned)(n0 - b0 * T);
#pragma unroll 1
        for (int pass = 0; pass < UE_PIECES / (UE_WG * UE_UNROLL); ++pass) {
            const unsigned lb = (unsigned)(pass * UE_WG * UE_UNROLL + tid);
            const long pb = p0 + lb;
            long lab[UE_UNROLL], urow[UE_UNROLL];
            int q[UE_UNROLL];
#pragma unroll
            for (int j = 0; j < UE_UNROLL; ++j) {
                const long p = pb + (long)j * UE_WG;
                lab[j] = -1;
                urow[j] = 0;
                q[j] = 0;
                if (p < pieces) {
                    const unsigned x = r0 + lb + (unsigned)(j * UE_WG), dn = x / (unsigned)qpr;
                    q[j] = (int)(x - dn * (unsigned)qpr);
                    const unsigned tt = t0 + dn, db = tt / (unsigned)T;
                    const long n = n0 + dn, b = b0 + db;
                    urow[j] = b;
                    if ((int64_t)(tt - db * (unsigned)T) < length[b]) {
                        const int64_t v = ind[n];
                        if (v >= 0 && v < K) lab[j] = (long)v;
                    }
                }
            }
            f32x4 v[UE_UNROLL], g[UE_UNROLL];
#pragma unroll
            for (int j = 0; j < UE_UNROLL; ++j) {
                v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
                g[j] = v[j];
                if (lab[j] >= 0) {
                    v[j] = *(const f32x4*)(table + ((size_t)lab[j] * qpr + q[j]) * 4);
                    if (glob) g[j] = *(const f32x4*)(glob + ((size_t)urow[j] * qpr + q[j]) * 4);
                }
            }
#pragma unroll
            for (int j = 0; j < UE_UNROLL; ++j) {
                const long p = pb + (long)j * UE_WG;
                if (p >= pieces) continue;
                f32x4 o = v[j];
                if (glob && lab[j] >= 0) o = o + g[j];
                *(f32x4*)(out + (size_t)p * 4) = o;
            }
        }
    }
}

__global__ __launch_bounds__(256) void ue_mask_kernel(const int64_t* __restrict__ ind, const int64_t* __restrict__ length,
                                                     int64_t* __restrict__ lab, int64_t* __restrict__ ulab, int N, int T, int K) {
    const long n = (long)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const int b = (int)(n / T), t = (int)(n - (long)b * T);
    int64_t v = -1, u = -1;
    if ((int64_t)t < length[b]) {
        const int64_t w = ind[n];
        if (w >= 0 && w < K) {
            v = w;
            u = b;
        }
    }
    lab[n] = v;
    ulab[n] = u;
}

static inline bool ue_takes(int B, int T, int C, int K) { return C >= 8 && C <= 2048 && C % 8 == 0 && K >= 1 && B >= 1 && T >= 1; }
static inline size_t ue_round16(size_t bytes) { return (bytes + 15) / 16 * 16; }

// N = B T where the backward takes the sizes, 0 otherwise
static int ue_frames(int B, int T, int C, int K) {
    if (!ue_takes(B, T, C, K)) return 0;
    const long N = (long)B * T;
    if ((double)N * C * 4.0 >= 4294967296.0) return 0;
    return (int)N;
}

struct ue_plan {
    size_t lab, counts, stats, bytes;
};

static ue_plan ue_make_plan(int N, int C, int K, int B) {
    ue_plan pl;
    pl.lab = ue_round16((size_t)N * sizeof(int64_t));
    pl.counts = ue_round16((size_t)(K > B ? K : B) * sizeof(float));
    const size_t sk = km_make_plan(N, C, K).bytes, sb = km_make_plan(N, C, B).bytes;
    pl.stats = sk > sb ? sk : sb;
    pl.bytes = 2 * pl.lab + pl.counts + pl.stats;
    return pl;
}

extern "C" {

int msmc_units_embed_fwd(const int64_t* ind, const int64_t* length, const float* table, const float* glob, float* out, int B, int T,
                         int C, int K, msmc_stream stream) {
    if (!ue_takes(B, T, C, K)) return MSMC_E_SHAPE;
    if ((((uintptr_t)table | (uintptr_t)glob | (uintptr_t)out) & 15) != 0) return MSMC_E_SHAPE;
    const int qpr = C >> 2;
    const long pieces = (long)B * T * qpr, blocks = (pieces + UE_PIECES - 1) / UE_PIECES;
    const long grid = blocks < 8L * MSMC_NUM_CU ? blocks : 8L * MSMC_NUM_CU;
    MSMC_LAUNCH(ue_fwd_kernel, dim3((unsigned)grid), dim3(UE_WG), 0, (msmc_stream_t)stream, ind, length, table, glob, out, pieces,
                blocks, T, qpr, K);
    return msmc_check_launch();
}

size_t msmc_units_embed_workspace(int N, int C, int K) {
    // (B <= N: the plan for B = N labels covers every batch of N frames)
    if (N < 1 || !ue_frames(N, 1, C, K)) return 0;
    return ue_make_plan(N, C, K, N).bytes;
}

int msmc_units_embed_bwd(const float* gout, const int64_t* ind, const int64_t* length, float* gtable, float* gglob, void* workspace,
                         size_t workspace_bytes, int B, int T, int C, int K, msmc_stream stream) {
    const int N = ue_frames(B, T, C, K);
    if (!N) return MSMC_E_SHAPE;
    if ((((uintptr_t)gout | (uintptr_t)gtable | (uintptr_t)gglob | (uintptr_t)workspace) & 15) != 0) return MSMC_E_SHAPE;
    const ue_plan pl = ue_make_plan(N, C, K, B);
    char* ws = (char*)workspace;
    int rc = km_stats_check(gout, gtable, ws + 2 * pl.lab + pl.counts, N, C, K);
    if (!rc && gglob) rc = km_stats_check(gout, gglob, ws + 2 * pl.lab + pl.counts, N, C, B);
    if (rc) return rc;
    if (!workspace || workspace_bytes < pl.bytes) return MSMC_E_WORKSPACE;
    msmc_stream_t st = (msmc_stream_t)stream;
    int64_t* lab = (int64_t*)ws;
    int64_t* ulab = (int64_t*)(ws + pl.lab);
    float* counts = (float*)(ws + 2 * pl.lab);
    void* sws = ws + 2 * pl.lab + pl.counts;
    MSMC_LAUNCH(ue_mask_kernel, dim3((unsigned)((N + 255L) / 256)), dim3(256), 0, st, ind, length, lab, ulab, N, T, K);
    rc = km_stats_launch(gout, lab, gtable, counts, sws, pl.stats, N, C, K, 0, st);
    if (rc || !gglob) return rc;
    return km_stats_launch(gout, ulab, gglob, counts, sws, pl.stats, N, C, B, 0, st);
}

}  // extern "C"
