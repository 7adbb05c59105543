// kmeans.hip -- the M step of Lloyd's algorithm at k-means unit widths (d = 768 / 1024, K = 100 .. 2000) for gfx950:
// per-centroid sums and counts of labelled frames (msmc_kmeans_stats) and the centre update (msmc_kmeans_update).
// The E step is msmc_vq_prepare + msmc_vq_search_wide (vq_wide.inc); the loop is msmctts_amd/hip/kmeans.py.
//
// The EMA statistics kernel (vq.hip vq_stats_kernel) writes one [K][d] partial per 16-frame tile and stops at d = 512.  Here
// the frames are grouped by centroid first (a stable counting sort of the frame numbers: 8 bytes read per frame), and the
// sums then read every row of x exactly once with 16-byte loads.  No floating-point atomics; the only atomics are integer
// adds on LDS counters.
//
// SUMMATION ORDER (restated in numpy by tests/_kmeansfitcases.py, compared bit for bit).  The rows of centroid k, in
// ascending frame number, are cut into runs of KM_RUN = 64 rows (the last run of a centroid may be shorter).  Per channel:
//     run partial  = (((+0 + x[n_0]) + x[n_1]) + ...)           the rows of the run in ascending n
//     total[k]     = (((+0 + partial_0) + partial_1) + ...)     the runs of the centroid in ascending order
//     sums[k]      = total[k]                (accumulate = 0)   |   sums[k] + total[k]              (accumulate = 1)
//     counts[k]    = (float)rows of k        (accumulate = 0)   |   counts[k] + (float)rows of k    (accumulate = 1)
// An empty centroid has total +0 and count 0 (with accumulate its sums and counts get that +0 added: one add per element
// for every centroid).  Entries of ind outside [0, K) are skipped by every step.  Plain IEEE adds (-ffp-contract=off).
//
// Launches of msmc_kmeans_stats (the frames are cut into P <= 256 parts of whole 256-frame tiles, P * K <= N + K):
//   km_hist_kernel       part p counts its frames per centroid in LDS -> cntp[p][k]
//   km_part_scan_kernel  per centroid: exclusive scan of cntp[.][k] over the parts (in place), the total -> off[k]
//   km_offsets_kernel    exclusive scans over k of the totals (off: first slot of centroid k in `order`) and of the run
//                        counts ceil(total / 64) (roff: first run of centroid k); off[K] / roff[K] hold the grand totals
//   km_place_kernel      part p walks its frames in ascending order, a tile of 256 at a time; a frame's slot is
//                        off[k] + (frames of k in earlier parts and tiles) + (frames of k before it in its tile): stable
//   km_stats_kernel      one workgroup per (run, slice of 1024 channels), a work-item per 4 channels: the run partial
//   km_reduce_kernel     a work-item per (centroid, 4 channels): total, sums, counts
// Workspace: ints cntp [P][K], off [K + 1], roff [K + 1], order [N], then floats partial [N / 64 + min(K, N)][d] -- an upper
// bound of the number of runs, known on the host without a read-back; workgroups of km_stats_kernel beyond roff[K] return.
//
// msmc_kmeans_update: one wave per centroid.  centers[k][c] = sums[k][c] / counts[k] (IEEE division) where counts[k] > 0, the
// row untouched otherwise.  shift2[k]: lane l sums (new - old)^2 of its channels in ascending order -- the 4-channel pieces
// l, l + 64, l + 128, ... and the four channels of a piece in order, from +0 -- then the 64 lane sums are added as a
// butterfly, v = v + v[lane ^ m] for m = 1, 2, 4, 8, 16, 32; +0 for an empty centroid.
#include <msmc_rt.hpp>
#include <msmc_hip.h>

#include "kmeans_stats.inc"        // the statistics kernels and km_stats_launch (shared with ema_wide.hip)

__global__ __launch_bounds__(64) void km_update_kernel(const float* __restrict__ sums, const float* __restrict__ counts,
                                                      float* __restrict__ centers, float* __restrict__ shift2, int d) {
    const size_t k = blockIdx.x;
    const int lane = threadIdx.x;
    const float n = counts[k];
    float s = 0.f;
    if (n > 0.f) {
        for (int q = lane; q < (d >> 2); q += 64) {
            const f32x4 t = *(const f32x4*)(sums + k * d + 4 * q);
            f32x4* row = (f32x4*)(centers + k * d + 4 * q);
            const f32x4 o = *row;
            f32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = t[j] / n;
                float df = v[j] - o[j];
                float sq = df * df;
                s = s + sq;
            }
            *row = v;
        }
    }
    s = wave_sum(s);
    if (lane == 0) shift2[k] = s;
}

extern "C" {

size_t msmc_kmeans_stats_workspace(int N, int d, int K) {
    if (km_bad_shape(d, K) || N <= 0) return 0;
    return km_make_plan(N, d, K).bytes;
}

int msmc_kmeans_stats(const float* x, const int64_t* ind, float* sums, float* counts, void* ws, size_t ws_bytes, int N, int d,
                      int K, int accumulate, msmc_stream stream) {
    const int rc = km_stats_check(x, sums, ws, N, d, K);
    if (rc) return rc;
    return km_stats_launch(x, ind, sums, counts, ws, ws_bytes, N, d, K, accumulate, (msmc_stream_t)stream);
}

int msmc_kmeans_update(const float* sums, const float* counts, float* centers, float* shift2, int d, int K, msmc_stream stream) {
    if (km_bad_shape(d, K)) return MSMC_E_SHAPE;
    if ((((uintptr_t)sums | (uintptr_t)centers) & 15) != 0) return MSMC_E_SHAPE;
    MSMC_LAUNCH(km_update_kernel, dim3((unsigned)K), dim3(64), 0, (msmc_stream_t)stream, sums, counts, centers, shift2, d);
    return msmc_check_launch();
}

}  // extern "C"
