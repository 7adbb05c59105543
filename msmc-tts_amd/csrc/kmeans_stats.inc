// kmeans_stats.inc -- the per-centroid statistics pass (counting sort by centroid, runs of 64 rows, fixed-order reduction),
// defined once: msmc_kmeans_stats (kmeans.hip) and the wide EMA update (ema_wide.hip) run the same kernels through
// km_stats_launch.  Summation order, launches and workspace layout: the head of kmeans.hip.  The kernels have internal
// linkage: every translation unit that includes this file carries its own copy.
#pragma once

#define KM_RUN 64            // rows per run
#define KM_PARTS 256         // most parts of the counting sort
#define KM_TILE 256          // frames per placement tile (= work-items of a workgroup)
#define KM_HIST 4096         // LDS counters per histogram pass
#define KM_MAX_D 2048

static __global__ __launch_bounds__(256) void km_hist_kernel(const int64_t* __restrict__ ind, int* __restrict__ cntp, int N,
                                                            int K, int part) {
    __shared__ int h[KM_HIST];
    const int p = blockIdx.x, tid = threadIdx.x;
    const long n0 = (long)p * part, n1 = n0 + part < N ? n0 + part : N;
    for (long k0 = 0; k0 < K; k0 += KM_HIST) {             // (K <= 4096: one pass over the part's labels)
        const int kn = K - k0 < KM_HIST ? (int)(K - k0) : KM_HIST;
        for (int i = tid; i < kn; i += 256) h[i] = 0;
        __syncthreads();
        for (long n = n0 + tid; n < n1; n += 256) {
            const int64_t v = ind[n];
            if (v >= k0 && v < k0 + kn) atomicAdd(&h[(int)(v - k0)], 1);
        }
        __syncthreads();
        for (int i = tid; i < kn; i += 256) cntp[(size_t)p * K + k0 + i] = h[i];
        __syncthreads();
    }
}

static __global__ __launch_bounds__(256) void km_part_scan_kernel(int* __restrict__ cntp, int* __restrict__ off, int P, int K) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    int run = 0;
#pragma unroll 8
    for (int p = 0; p < P; ++p) {
        const int c = cntp[(size_t)p * K + k];
        cntp[(size_t)p * K + k] = run;
        run += c;
    }
    off[k] = run;
}

// one workgroup; in: off[k] = rows of centroid k; out: off / roff as described at the top of kmeans.hip
static __global__ __launch_bounds__(256) void km_offsets_kernel(int* __restrict__ off, int* __restrict__ roff, int K) {
    __shared__ int so[256], sr[256];
    const int tid = threadIdx.x;
    const long chunk = ((long)K + 255) / 256;
    const long k0 = tid * chunk < K ? tid * chunk : K, k1 = k0 + chunk < K ? k0 + chunk : K;
    int a = 0, r = 0;
    for (long k = k0; k < k1; ++k) {
        const int c = off[k];
        a += c;
        r += (c + KM_RUN - 1) / KM_RUN;
    }
    so[tid] = a;
    sr[tid] = r;
    __syncthreads();
    if (tid == 0) {
        int ta = 0, tr = 0;
        for (int i = 0; i < 256; ++i) {
            const int ca = so[i], cr = sr[i];
            so[i] = ta;
            sr[i] = tr;
            ta += ca;
            tr += cr;
        }
        off[K] = ta;
        roff[K] = tr;
    }
    __syncthreads();
    a = so[tid];
    r = sr[tid];
    for (long k = k0; k < k1; ++k) {
        const int c = off[k];
        off[k] = a;
        roff[k] = r;
        a += c;
        r += (c + KM_RUN - 1) / KM_RUN;
    }
}

static __global__ __launch_bounds__(256) void km_place_kernel(const int64_t* __restrict__ ind, const int* __restrict__ off,
                                                             int* cntp, int* __restrict__ order, int N, int K, int part) {
    __shared__ __attribute__((aligned(16))) int sk[KM_TILE];
    const int p = blockIdx.x, tid = threadIdx.x;
    int* placed = cntp + (size_t)p * K;          // rows of centroid k in the parts before this one, plus this part's earlier tiles
    const long n0 = (long)p * part, n1 = n0 + part < N ? n0 + part : N;
    for (long t0 = n0; t0 < n1; t0 += KM_TILE) {
        const long n = t0 + tid;
        int k = -1;
        if (n < n1) {
            const int64_t v = ind[n];
            if (v >= 0 && v < K) k = (int)v;
        }
        sk[tid] = k;
        __syncthreads();
        int rank = 0, tot = 0;                   // frames of k before this one in the tile / in the whole tile
        for (int j = 0; j < KM_TILE; j += 4) {
            const u32x4 v = *(const u32x4*)(sk + j);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int m = (int)v[i] == k ? 1 : 0;
                tot += m;
                rank += j + i < tid ? m : 0;
            }
        }
        int at = 0;
        if (k >= 0) {
            at = placed[k];
            order[(size_t)off[k] + at + rank] = (int)n;
        }
        __syncthreads();                         // every frame of the tile has read placed[k] ...
        if (k >= 0 && rank == tot - 1) placed[k] = at + tot;
        __syncthreads();                         // ... and the next tile reads what the last frame of k left
    }
}

static __global__ __launch_bounds__(256) void km_stats_kernel(const float* __restrict__ x, const int* __restrict__ off,
                                                             const int* __restrict__ roff, const int* __restrict__ order,
                                                             float* __restrict__ partial, int d, int K) {
    const int r = blockIdx.x;
    if (r >= roff[K]) return;
    // the centroid of run r: roff[k] <= r < roff[k + 1] (empty centroids have no run and are passed over)
    int k = 0, hi = K;
    while (hi - k > 1) {
        const int mid = k + (hi - k) / 2;
        if (roff[mid] <= r) k = mid;
        else hi = mid;
    }
    const int c = 4 * ((int)blockIdx.y * 256 + (int)threadIdx.x);
    if (c >= d) return;
    const int first = off[k] + (r - roff[k]) * KM_RUN;
    const int len = off[k + 1] - first < KM_RUN ? off[k + 1] - first : KM_RUN;
    const int* rows = order + first;
    const float* xc = x + c;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    int i = 0;
    for (; i + 8 <= len; i += 8) {               // eight rows in flight, added in ascending order
        f32x4 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = *(const f32x4*)(xc + (size_t)rows[i + j] * d);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc = acc + v[j];
    }
    for (; i < len; ++i) acc = acc + *(const f32x4*)(xc + (size_t)rows[i] * d);
    *(f32x4*)(partial + (size_t)r * d + c) = acc;
}

static __global__ __launch_bounds__(256) void km_reduce_kernel(const float* __restrict__ partial, const int* __restrict__ off,
                                                              const int* __restrict__ roff, float* sums, float* counts, int d,
                                                              int accumulate, long total) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int dv = d >> 2;
    const long k = e / dv;
    const int c = 4 * (int)(e - k * dv);
    const int r0 = roff[k], r1 = roff[k + 1];
    f32x4 t = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int r = r0; r < r1; ++r) t = t + *(const f32x4*)(partial + (size_t)r * d + c);
    f32x4* dst = (f32x4*)(sums + (size_t)k * d + c);
    if (accumulate) t = *dst + t;
    *dst = t;
    if (c == 0) {
        const float n = (float)(off[k + 1] - off[k]);
        counts[k] = accumulate ? counts[k] + n : n;
    }
}

static __global__ __launch_bounds__(256) void km_zero_kernel(float* __restrict__ p, long n) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) p[e] = 0.f;
}

struct km_plan {
    int P, part;                 // parts of the counting sort, frames per part (whole tiles)
    size_t ints;                 // cntp, off, roff, order
    size_t runs;                 // upper bound of the number of runs
    size_t bytes;
};

static km_plan km_make_plan(int N, int d, int K) {
    km_plan pl;
    long P = (long)N / K;
    if (P > KM_PARTS) P = KM_PARTS;
    if (P > ((long)N + KM_TILE - 1) / KM_TILE) P = ((long)N + KM_TILE - 1) / KM_TILE;
    if (P < 1) P = 1;
    long part = ((long)N + P - 1) / P;
    part = (part + KM_TILE - 1) / KM_TILE * KM_TILE;
    pl.part = (int)part;
    pl.P = (int)(((long)N + part - 1) / part);
    pl.ints = (size_t)pl.P * K + 2 * ((size_t)K + 1) + (size_t)N;
    pl.runs = (size_t)N / KM_RUN + (size_t)(K < N ? K : N);
    pl.bytes = (pl.ints * sizeof(int) + 15) / 16 * 16 + pl.runs * d * sizeof(float);
    return pl;
}

static inline bool km_bad_shape(int d, int K) { return d < 4 || d > KM_MAX_D || d % 4 || K < 1; }

// 0 where km_stats_launch takes the arguments, MSMC_E_SHAPE otherwise (nothing is launched by either)
static int km_stats_check(const float* x, const float* sums, const void* ws, int N, int d, int K) {
    if (km_bad_shape(d, K) || N < 0) return MSMC_E_SHAPE;
    if ((double)N * d * 4.0 >= 4294967296.0) return MSMC_E_SHAPE;
    if ((((uintptr_t)x | (uintptr_t)sums | (uintptr_t)ws) & 15) != 0) return MSMC_E_SHAPE;
    if (((long)K * (d >> 2) + 255) / 256 > 0x7fffffffL) return MSMC_E_SHAPE;
    return 0;
}

// the launches of msmc_kmeans_stats on arguments km_stats_check passed
static int km_stats_launch(const float* x, const int64_t* ind, float* sums, float* counts, void* ws, size_t ws_bytes, int N,
                           int d, int K, int accumulate, msmc_stream_t st) {
    const long quads = (long)K * (d >> 2);
    if (N == 0) {
        if (accumulate) return 0;
        const long cap = 8L * MSMC_NUM_CU;
        const long bs = (4 * quads + 255) / 256 < cap ? (4 * quads + 255) / 256 : cap, bc = (K + 255L) / 256 < cap ? (K + 255L) / 256 : cap;
        MSMC_LAUNCH(km_zero_kernel, dim3((unsigned)bs), dim3(256), 0, st, sums, 4 * quads);
        MSMC_LAUNCH(km_zero_kernel, dim3((unsigned)bc), dim3(256), 0, st, counts, (long)K);
        return msmc_check_launch();
    }
    const km_plan pl = km_make_plan(N, d, K);
    if (!ws || ws_bytes < pl.bytes) return MSMC_E_WORKSPACE;
    int* cntp = (int*)ws;
    int* off = cntp + (size_t)pl.P * K;
    int* roff = off + (size_t)K + 1;
    int* order = roff + (size_t)K + 1;
    float* partial = (float*)((char*)ws + (pl.ints * sizeof(int) + 15) / 16 * 16);
    MSMC_LAUNCH(km_hist_kernel, dim3(pl.P), dim3(256), 0, st, ind, cntp, N, K, pl.part);
    MSMC_LAUNCH(km_part_scan_kernel, dim3((unsigned)((K + 255L) / 256)), dim3(256), 0, st, cntp, off, pl.P, K);
    MSMC_LAUNCH(km_offsets_kernel, dim3(1), dim3(256), 0, st, off, roff, K);
    MSMC_LAUNCH(km_place_kernel, dim3(pl.P), dim3(256), 0, st, ind, off, cntp, order, N, K, pl.part);
    MSMC_LAUNCH(km_stats_kernel, dim3((unsigned)pl.runs, (d + 1023) / 1024), dim3(256), 0, st, x, off, roff, order, partial, d, K);
    MSMC_LAUNCH(km_reduce_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, st, partial, off, roff, sums, counts, d,
                accumulate, quads);
    return msmc_check_launch();
}
