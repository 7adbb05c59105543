// ema_wide.hip -- the EMA codebook update of ONE wide head (d % 16 == 0, 16 <= d <= 2048, any K >= 1: the shapes of the wide
// search, wide_tile.inc wide_takes) for gfx950: the k-means unit codebooks (d = 768 / 1024, K = 100 .. 2000) trained online.
// The resident EMA kernels (vq.hip) stage a tile's rows in LDS and keep one [K][d] partial per tile: they stop at d = 512.
// Here the statistics are those of the k-means M step -- the counting sort and the 64-row runs of kmeans_stats.inc on labels
// masked by the utterance lengths -- and the update reads the [K][d] sums once, transposing 64 x 64 tiles through LDS into the
// reference's [d][K] buffers.
//
// ORDER OF EVERY OPERATION (restated in numpy by tests/_emawidecases.py, compared bit for bit; -ffp-contract=off):
//   lab[n]        = ind[n] where t < length[b] (n = b T + t), else -1: skipped by the statistics, its row of x never read
//   sums, counts  = msmc_kmeans_stats of (x, lab) without accumulate: runs of 64 rows in ascending n, head of kmeans.hip
//   omd           = (float)(1.0 - (double)decay),  keps = (float)((double)K * (double)eps)
//   cs_new[k]     = fmaf(+0 + counts[k], omd, cluster_size[k] * decay)                 the arithmetic of vq_ema_cs_kernel
//   n             = sum of cs_new in the order of vq_ema_kernel: p[t] = ((+0 + cs_new[t]) + cs_new[t + 256]) + ... for
//                   t = 0 .. 255, then p[t] = p[t] + p[t + s] for t < s, s = 128, 64, .. 1; n = p[0]
//   sm[k]         = (cs_new[k] + eps) / (n + keps) * n                                 three roundings, left to right
//   embed_avg[j][k] = fmaf(sums[k][j], omd, embed_avg[j][k] * decay);  embed[j][k] = embed_avg[j][k] / sm[k]   (IEEE division)
//   cluster_size[k] = cs_new[k]
// Same inputs, same bits: no floating-point atomics, and every workgroup of the update derives the same n.
//
// Launches:  ew_mask_kernel, the six of km_stats_launch (_stats);  ew_cs_kernel, ew_apply_kernel (_apply).
// ew_apply_kernel: grid (ceil(K / 64), ceil(d / 64)), one [64 k][64 channel] tile per workgroup.  The tile of sums comes in with
// 16-byte loads along the channels and is stored transposed, tile[channel][k] with a pitch of 65 words; embed_avg / embed are
// read and written with k fastest (256 contiguous bytes per wave).  LDS banking (ds_write_b32 / ds_read_b32: 32 banks, lanes
// conflict within a 32-lane half): a half wave stores 8 channel quads x 4 rows, word (4 q + e) 65 + r -> bank (4 q + e + r) % 32,
// all 32 distinct; the transposed reads are 32 consecutive words.  Tiles that end past K or d are predicated (d % 16 == 0: a
// 16-byte piece is inside or outside as a whole).
// Workspace of _stats / _update: int64 lab [N] (rounded up to 16 bytes), the workspace of msmc_kmeans_stats, and for _update the
// stats block [K][d] sums, [K] counts, [K] cs_new.
#include <msmc_rt.hpp>
#include <msmc_hip.h>

#include "kmeans_stats.inc"

#define EW_TILE 64
#define EW_PITCH 65

__global__ __launch_bounds__(256) void ew_mask_kernel(const int64_t* __restrict__ ind, const int64_t* __restrict__ length,
                                                     int64_t* __restrict__ lab, int N, int T) {
    const long n = (long)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const int b = (int)(n / T), t = (int)(n - (long)b * T);
    int64_t v = -1;
    if ((int64_t)t < length[b]) v = ind[n];
    lab[n] = v;
}

__global__ __launch_bounds__(256) void ew_cs_kernel(const float* __restrict__ counts, const float* __restrict__ cluster_size,
                                                   float* __restrict__ cs_new, int K, float decay, float omd) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    float c = 0.f;
    c = c + counts[k];
    float v = cluster_size[k] * decay;
    cs_new[k] = fmaf(c, omd, v);
}

__global__ __launch_bounds__(256) void ew_apply_kernel(const float* __restrict__ sums, const float* __restrict__ cs_new,
                                                      float* __restrict__ embed, float* __restrict__ cluster_size,
                                                      float* __restrict__ embed_avg, int d, int K, float decay, float omd,
                                                      float eps, float keps) {
    __shared__ float tile[EW_TILE * EW_PITCH];   // [channel][k]
    __shared__ float red[256];
    __shared__ float ssm[EW_TILE];
    const int tid = threadIdx.x;
    const long k0 = (long)blockIdx.x * EW_TILE;
    const int j0 = (int)blockIdx.y * EW_TILE;
    // the tile of sums: wave w, pass `it` takes rows 16 it + 4 w .. + 3; a half wave covers 8 quads of 4 rows
    const int lane = tid & 63, w = tid >> 6;
    const int q = (lane & 7) + 8 * (lane >> 5), rr = (lane >> 3) & 3;
    f32x4 v[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int r = 16 * it + 4 * w + rr;
        v[it] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (k0 + r < K && j0 + 4 * q < d) v[it] = *(const f32x4*)(sums + (size_t)(k0 + r) * d + j0 + 4 * q);
    }
    // n, in the order of vq_ema_kernel
    float p = 0.f;
    for (long k = tid; k < K; k += 256) p = p + cs_new[k];
    red[tid] = p;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int r = 16 * it + 4 * w + rr;
#pragma unroll
        for (int e = 0; e < 4; ++e) tile[(4 * q + e) * EW_PITCH + r] = v[it][e];
    }
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    const float n = red[0];
    const float den = n + keps;
    if (tid < EW_TILE && k0 + tid < K) {
        const float c = cs_new[k0 + tid];
        float sm = (c + eps) / den * n;
        ssm[tid] = sm;
        if (blockIdx.y == 0) cluster_size[k0 + tid] = c;
    }
    __syncthreads();
    const long k = k0 + lane;
    if (k >= K) return;
    const float sm = ssm[lane];
#pragma unroll 4
    for (int it = 0; it < 16; ++it) {
        const int c = 4 * it + w;
        if (j0 + c >= d) break;
        const float s = tile[c * EW_PITCH + lane];
        const size_t o = (size_t)(j0 + c) * K + k;
        float a = embed_avg[o] * decay;
        a = fmaf(s, omd, a);
        embed_avg[o] = a;
        embed[o] = a / sm;
    }
}

// the shapes of the wide search (wide_tile.inc wide_takes)
static inline bool ew_takes(int d, int K) { return d >= 16 && d <= 2048 && d % 16 == 0 && K >= 1; }
static inline size_t ew_lab_bytes(long N) { return ((size_t)N * sizeof(int64_t) + 15) / 16 * 16; }

// N = B T where _stats takes the sizes, 0 otherwise
static int ew_frames(int B, int T, int d, int K) {
    if (!ew_takes(d, K) || B < 1 || T < 1) return 0;
    const long N = (long)B * T;
    if ((double)N * d * 4.0 >= 4294967296.0) return 0;
    return (int)N;
}

static int ew_stats(const float* x, const int64_t* ind, const int64_t* length, float* stats, void* ws, size_t ws_bytes, int N,
                    int T, int d, int K, msmc_stream_t st) {
    int64_t* lab = (int64_t*)ws;
    const size_t lb = ew_lab_bytes(N);
    MSMC_LAUNCH(ew_mask_kernel, dim3((unsigned)((N + 255L) / 256)), dim3(256), 0, st, ind, length, lab, N, T);
    return km_stats_launch(x, lab, stats, stats + (size_t)K * d, (char*)ws + lb, ws_bytes - lb, N, d, K, 0, st);
}

static int ew_apply(float* stats, float* embed, float* cluster_size, float* embed_avg, int d, int K, float decay, float eps,
                    msmc_stream_t st) {
    const float omd = (float)(1.0 - (double)decay);
    const float keps = (float)((double)K * (double)eps);
    const float* counts = stats + (size_t)K * d;
    float* cs_new = stats + (size_t)K * d + K;
    MSMC_LAUNCH(ew_cs_kernel, dim3((unsigned)((K + 255L) / 256)), dim3(256), 0, st, counts, (const float*)cluster_size, cs_new, K,
                decay, omd);
    int rc = msmc_check_launch();
    if (rc) return rc;
    MSMC_LAUNCH(ew_apply_kernel, dim3((unsigned)((K + EW_TILE - 1L) / EW_TILE), (d + EW_TILE - 1) / EW_TILE), dim3(256), 0, st,
                (const float*)stats, (const float*)cs_new, embed, cluster_size, embed_avg, d, K, decay, omd, eps, keps);
    return msmc_check_launch();
}

extern "C" {

size_t msmc_vq_ema_wide_workspace(int N, int d, int K) {
    if (N < 1 || !ew_frames(N, 1, d, K)) return 0;
    return ew_lab_bytes(N) + km_make_plan(N, d, K).bytes + (size_t)K * ((size_t)d + 2) * sizeof(float);
}

int msmc_vq_ema_wide_stats(const float* x, const int64_t* ind, const int64_t* length, float* stats, void* workspace,
                           size_t workspace_bytes, int B, int T, int d, int K, msmc_stream stream) {
    const int N = ew_frames(B, T, d, K);
    if (!N) return MSMC_E_SHAPE;
    if ((((uintptr_t)x | (uintptr_t)stats | (uintptr_t)workspace) & 15) != 0) return MSMC_E_SHAPE;
    const size_t lb = ew_lab_bytes(N);
    const int rc = km_stats_check(x, stats, (char*)workspace + lb, N, d, K);
    if (rc) return rc;
    if (!workspace || workspace_bytes < lb + km_make_plan(N, d, K).bytes) return MSMC_E_WORKSPACE;
    return ew_stats(x, ind, length, stats, workspace, workspace_bytes, N, T, d, K, (msmc_stream_t)stream);
}

int msmc_vq_ema_wide_apply(float* stats, float* embed, float* cluster_size, float* embed_avg, int d, int K, float decay,
                           float eps, msmc_stream stream) {
    if (!ew_takes(d, K) || ((uintptr_t)stats & 15) != 0) return MSMC_E_SHAPE;
    return ew_apply(stats, embed, cluster_size, embed_avg, d, K, decay, eps, (msmc_stream_t)stream);
}

int msmc_vq_ema_wide_update(const float* x, const int64_t* ind, const int64_t* length, float* embed, float* cluster_size,
                            float* embed_avg, void* workspace, size_t workspace_bytes, int B, int T, int d, int K, float decay,
                            float eps, msmc_stream stream) {
    const int N = ew_frames(B, T, d, K);
    if (!N) return MSMC_E_SHAPE;
    if ((((uintptr_t)x | (uintptr_t)workspace) & 15) != 0) return MSMC_E_SHAPE;
    const size_t lb = ew_lab_bytes(N), kb = km_make_plan(N, d, K).bytes;
    float* stats = (float*)((char*)workspace + lb + kb);
    int rc = km_stats_check(x, stats, (char*)workspace + lb, N, d, K);
    if (rc) return rc;
    if (!workspace || workspace_bytes < lb + kb + (size_t)K * ((size_t)d + 2) * sizeof(float)) return MSMC_E_WORKSPACE;
    rc = ew_stats(x, ind, length, stats, workspace, lb + kb, N, T, d, K, (msmc_stream_t)stream);
    if (rc) return rc;
    return ew_apply(stats, embed, cluster_size, embed_avg, d, K, decay, eps, (msmc_stream_t)stream);
}

}  // extern "C"
