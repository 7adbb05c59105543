// kmeans_pp.hip -- greedy k-means++ seeding (Arthur & Vassilvitskii, with scikit-learn's local trials) of the k-means unit
// codebook for gfx950: msmc_kmeanspp_seed picks K frames of x [N, d] as the first centres of Lloyd's algorithm
// (msmctts_amd/hip/kmeans.py: kmeans_plusplus, fit_kmeans(init='k-means++')).  The whole seeding is enqueued at once: two
// launches per centre, nothing read back; candidates, the winner and the tile prefixes stay in the workspace.
//
// ALGORITHM.  L candidates per step, uniforms u [K - 1][L] in [0, 1) from the caller.
//     centre 0 = x[first];  mind[n] = |x[n] - centre 0|^2
//     step i = 1 .. K - 1:  candidate j = the first frame n with cum[n] > u[i - 1][j] * total     (cum: running sum of mind)
//                           pot[j]      = sum over n of min(mind[n], |x[n] - x[candidate j]|^2)
//                           the candidate of the smallest pot wins (ties: the lowest j); its row is centre i, mind takes the
//                           minimum with its distances, potential[i] = pot[winner]            (potential[0] = sum of mind)
//
// ORDER OF EVERY SUM (restated in numpy by tests/_kmeansppcases.py, compared bit for bit; plain IEEE, -ffp-contract=off).
//   distance   fp32, the direct difference: lane l of a 64-lane wave adds (x - c)^2 of the 4-channel pieces l, l + 64, ...
//              in ascending channel order from +0 (difference, square, add: three roundings), then the 64 lane sums are
//              added as the butterfly of wave_sum, v = v + v[lane ^ m] for m = 1, 2, 4, 8, 16, 32 -- the order of shift2 in
//              msmc_kmeans_update.  A frame is at distance +0 from itself, so a chosen frame has weight 0.
//   minimum    a < b ? a : b in fp32.
//   tile sum   the frames are cut into tiles of KPP_TILE = 256 (the last may be shorter); per candidate and tile
//              local[n] = (((+0 + m[n0]) + m[n0 + 1]) + ... + m[n]) in float64, m = the fp32 minima of the tile in ascending n;
//              the tile's partial is local of its last frame.
//   prefix     pre[0] = +0, pre[t + 1] = pre[t] + partial[t] in float64, tiles in ascending order; pot = total = pre[T].
//   cum        cum[n] = pre[t] + local[n] for n in tile t.  It never decreases, and cum[N - 1] is total bit for bit (the
//              winner's partials ARE the next step's tile sums), so for total > 0 and u < 1 a pick exists and a frame of
//              weight 0 is never picked (strict >).  threshold = u * total, one float64 product.
//   total == 0 (every frame coincides with a centre) or no pick: frame N - 1.
//
// Launches of msmc_kmeanspp_seed (T = ceil(N / 256) tiles):
//   kpp_dist_kernel     one workgroup per tile, the L candidate rows staged in LDS through their device-side frame numbers,
//                       one wave per two frames at a time with L accumulators each: x is read once per step with 16-byte
//                       loads.  Writes the minima min(mind, distance) [L][N] and the float64 tile partials [L][T].  Centre 0
//                       is the same launch with one candidate (first) and no mind.
//   kpp_select_kernel   one workgroup: the prefixes of every candidate (a work-item per candidate, tiles in chunks through
//                       LDS), the winner, its row -> centers, chosen, potential; then a work-item per candidate of the NEXT
//                       step: binary search of the winner's prefixes for the tile, a walk through that tile for the frame.
// The winner's row of minima is the next step's mind (two [L][N] buffers alternate): mind is never reduced a second time.
// Workspace: ints state[32] (candidates [16], winner), doubles pre [L][T + 1], part [L][T], floats minima 2 x [L][N].
#include <msmc_rt.hpp>
#include <msmc_hip.h>

#define KPP_TILE 256         // frames per tile (= work-items of a workgroup)
#define KPP_ROW 257          // floats per candidate in the LDS image of a tile's minima (odd: no bank conflicts down a column)
#define KPP_MAX_L 16
#define KPP_MAX_D 2048
#define KPP_STATE 32         // ints: the candidates' frame numbers [16], the winner [1]
#define KPP_BEST 16

template <int LMAX>
__global__ __launch_bounds__(256) void kpp_dist_kernel(const float* __restrict__ x, const int* __restrict__ state,
                                                      const float* prev, float* __restrict__ cur, double* __restrict__ part,
                                                      int N, int d, int T, int L) {
    MSMC_DYN_LDS(lds);
    float* cr = (float*)lds;                     // candidate rows [L][d]
    float* mv = cr + (size_t)L * d;              // distances, then minima, of the tile [L][KPP_ROW]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int dv = d >> 2;
    for (int e = tid; e < L * dv; e += 256) {
        const int j = e / dv, q = e - j * dv;
        *(f32x4*)(cr + 4 * (size_t)e) = *(const f32x4*)(x + (size_t)state[j] * d + 4 * q);
    }
    __syncthreads();
    const long n0 = (long)blockIdx.x * KPP_TILE;
    const int cnt = N - n0 < KPP_TILE ? (int)(N - n0) : KPP_TILE;
    for (int i = 0; i < 64; i += 2) {
        const int fa = w * 64 + i;
        if (fa >= cnt) break;
        const int fb = fa + 1 < cnt ? fa + 1 : fa;       // (an odd last frame is computed twice, stored once)
        const float* xa = x + (size_t)(n0 + fa) * d;
        const float* xb = x + (size_t)(n0 + fb) * d;
        float sa[LMAX], sb[LMAX];
#pragma unroll
        for (int j = 0; j < LMAX; ++j) sa[j] = sb[j] = 0.f;
        for (int q0 = lane; q0 < dv + lane; q0 += 256) {  // four pieces of either frame in flight
            f32x4 va[4], vb[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int q = q0 + 64 * p;
                if (q < dv) {
                    va[p] = *(const f32x4*)(xa + 4 * q);
                    vb[p] = *(const f32x4*)(xb + 4 * q);
                }
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int q = q0 + 64 * p;
                if (q < dv) {
#pragma unroll
                    for (int j = 0; j < LMAX; ++j) {
                        if (j < L) {
                            const f32x4 c = *(const f32x4*)(cr + (size_t)j * d + 4 * q);
                            const f32x4 da = va[p] - c, db = vb[p] - c;
                            const f32x4 qa = da * da, qb = db * db;
#pragma unroll
                            for (int k = 0; k < 4; ++k) {
                                sa[j] = sa[j] + qa[k];
                                sb[j] = sb[j] + qb[k];
                            }
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < LMAX; ++j) {
            if (j < L) {
                const float ta = wave_sum(sa[j]), tb = wave_sum(sb[j]);
                if (lane == 0) {
                    mv[j * KPP_ROW + fa] = ta;
                    mv[j * KPP_ROW + fb] = tb;
                }
            }
        }
    }
    __syncthreads();
    if (tid < cnt) {
        const float m0 = prev ? prev[(size_t)state[KPP_BEST] * N + n0 + tid] : 0.f;
        for (int j = 0; j < L; ++j) {
            float v = mv[j * KPP_ROW + tid];
            if (prev) v = m0 < v ? m0 : v;
            mv[j * KPP_ROW + tid] = v;
            cur[(size_t)j * N + n0 + tid] = v;
        }
    }
    __syncthreads();
    if (tid < L) {
        double a = 0.0;
        for (int i = 0; i < cnt; ++i) a = a + (double)mv[tid * KPP_ROW + i];
        part[(size_t)tid * T + blockIdx.x] = a;
    }
}

// u: the uniforms [Lnext] of the next step (unused for Lnext == 0, after the last centre)
__global__ __launch_bounds__(256) void kpp_select_kernel(const float* __restrict__ x, const double* __restrict__ part, double* pre,
                                                        const float* __restrict__ cur, const double* __restrict__ u, int* state,
                                                        float* __restrict__ centers, int64_t* __restrict__ chosen,
                                                        double* __restrict__ potential, int N, int d, int T, int Lcur, int Lnext,
                                                        int step) {
    __shared__ double s[KPP_MAX_L][KPP_TILE + 1];
    __shared__ double pot[KPP_MAX_L];
    __shared__ int winner[2], tile_of[KPP_MAX_L];
    const int tid = threadIdx.x;
    const size_t T1 = (size_t)T + 1;
    // the prefixes, a chunk of 256 tiles at a time; the next chunk is requested before this one is walked
    double nx[KPP_MAX_L], run = 0.0;
#pragma unroll
    for (int j = 0; j < KPP_MAX_L; ++j) nx[j] = j < Lcur && tid < T ? part[(size_t)j * T + tid] : 0.0;
    for (long t0 = 0; t0 < T; t0 += KPP_TILE) {
        const int cn = T - t0 < KPP_TILE ? (int)(T - t0) : KPP_TILE;
#pragma unroll
        for (int j = 0; j < KPP_MAX_L; ++j)
            if (j < Lcur) s[j][tid] = nx[j];
        __syncthreads();
        const long t1 = t0 + KPP_TILE + tid;
#pragma unroll
        for (int j = 0; j < KPP_MAX_L; ++j)
            if (j < Lcur && t1 < T) nx[j] = part[(size_t)j * T + t1];
        if (tid < Lcur) {
            for (int i = 0; i < cn; ++i) {
                const double v = s[tid][i];
                s[tid][i] = run;
                run = run + v;
            }
        }
        __syncthreads();
        if (tid < cn)
            for (int j = 0; j < Lcur; ++j) pre[j * T1 + t0 + tid] = s[j][tid];
        __syncthreads();
    }
    if (tid < Lcur) {
        pre[tid * T1 + T] = run;
        pot[tid] = run;
    }
    __syncthreads();
    if (tid == 0) {
        int best = 0;
        for (int j = 1; j < Lcur; ++j)
            if (pot[j] < pot[best]) best = j;
        winner[0] = best;
        winner[1] = state[best];
        state[KPP_BEST] = best;
        chosen[step] = state[best];
        potential[step] = pot[best];
    }
    __syncthreads();                             // (orders the reads of the candidates before the picks overwrite them, and pre)
    const int best = winner[0];
    const float* row = x + (size_t)winner[1] * d;
    for (int q = tid; q < (d >> 2); q += 256) *(f32x4*)(centers + (size_t)step * d + 4 * q) = *(const f32x4*)(row + 4 * q);
    if (Lnext == 0) return;
    const double* p = pre + best * T1;
    const float* mind = cur + (size_t)best * N;
    double thr = 0.0;
    if (tid < Lnext) {                           // the candidate's tile: the first t with pre[t + 1] > thr, -1 without one
        const double total = p[T];
        long lo = -1;
        if (total > 0.0) {
            thr = u[tid] * total;
            if (total > thr) {
                long hi = (long)T - 1;
                lo = 0;
                while (lo < hi) {
                    const long mid = lo + (hi - lo) / 2;
                    if (p[mid + 1] > thr) hi = mid;
                    else lo = mid + 1;
                }
            }
        }
        tile_of[tid] = (int)lo;
    }
    __syncthreads();
    for (int j = 0; j < Lnext; ++j) {            // the minima of the candidates' tiles, fetched by the whole workgroup
        const long n = (long)tile_of[j] * KPP_TILE + tid;
        if (tile_of[j] >= 0 && n < N) s[j][tid] = (double)mind[n];
    }
    __syncthreads();
    if (tid < Lnext) {
        long pick = (long)N - 1;
        if (tile_of[tid] >= 0) {
            const long n0 = (long)tile_of[tid] * KPP_TILE;
            const int cn = N - n0 < KPP_TILE ? (int)(N - n0) : KPP_TILE;
            const double base = p[tile_of[tid]];
            double loc = 0.0;
            for (int i = 0; i < cn; ++i) {
                loc = loc + s[tid][i];
                if (base + loc > thr) {
                    pick = n0 + i;
                    break;
                }
            }
        }
        state[tid] = (int)pick;
    }
}

__global__ void kpp_first_kernel(int* state, int first) {
    if (threadIdx.x == 0) {
        state[0] = first;
        state[KPP_BEST] = 0;
    }
}

struct kpp_plan {
    int T;                       // tiles
    size_t pre, part, buf;       // byte offsets of pre, part and the first buffer of minima
    size_t buf_bytes, bytes;     // one buffer of minima; the workspace
};

static inline size_t kpp_up16(size_t v) { return (v + 15) / 16 * 16; }

static kpp_plan kpp_make_plan(int N, int L) {
    kpp_plan pl;
    pl.T = (int)(((long)N + KPP_TILE - 1) / KPP_TILE);
    pl.pre = KPP_STATE * sizeof(int);
    pl.part = pl.pre + kpp_up16((size_t)L * ((size_t)pl.T + 1) * sizeof(double));
    pl.buf = pl.part + kpp_up16((size_t)L * pl.T * sizeof(double));
    pl.buf_bytes = kpp_up16((size_t)L * N * sizeof(float));
    pl.bytes = pl.buf + 2 * pl.buf_bytes;
    return pl;
}

static inline bool kpp_bad_shape(int N, int d, int K, int L) {
    return d < 4 || d > KPP_MAX_D || d % 4 || K < 1 || L < 1 || L > KPP_MAX_L || N < 1;
}

static int kpp_launch_dist(const float* x, const int* state, const float* prev, float* cur, double* part, int N, int d, int T,
                           int L, msmc_stream_t st) {
    void (*fn)(const float*, const int*, const float*, float*, double*, int, int, int, int) =
        L == 1 ? kpp_dist_kernel<1> : L <= 8 ? kpp_dist_kernel<8> : kpp_dist_kernel<16>;
    const size_t lds = ((size_t)L * d + (size_t)L * KPP_ROW) * sizeof(float);
    const int rc = msmc_allow_lds((const void*)fn, (int)lds);
    if (rc) return rc;
    MSMC_LAUNCH(fn, dim3((unsigned)T), dim3(256), lds, st, x, state, prev, cur, part, N, d, T, L);
    msmc_prof_name("kpp_dist_kernel");
    return 0;
}

extern "C" {

size_t msmc_kmeanspp_workspace(int N, int d, int K, int L) {
    if (kpp_bad_shape(N, d, K, L)) return 0;
    return kpp_make_plan(N, L).bytes;
}

int msmc_kmeanspp_seed(const float* x, int N, int d, int K, int L, long first, const double* u, float* centers, int64_t* chosen,
                       double* potential, void* ws, size_t ws_bytes, msmc_stream stream) {
    if (kpp_bad_shape(N, d, K, L) || first < 0 || first >= N) return MSMC_E_SHAPE;
    if ((((uintptr_t)x | (uintptr_t)centers | (uintptr_t)ws) & 15) != 0) return MSMC_E_SHAPE;
    if ((((uintptr_t)u | (uintptr_t)chosen | (uintptr_t)potential) & 7) != 0) return MSMC_E_SHAPE;
    if (!x || !centers || !chosen || !potential || (K > 1 && !u)) return MSMC_E_SHAPE;
    const kpp_plan pl = kpp_make_plan(N, L);
    if (!ws || ws_bytes < pl.bytes) return MSMC_E_WORKSPACE;
    msmc_stream_t st = (msmc_stream_t)stream;
    int* state = (int*)ws;
    double* pre = (double*)((char*)ws + pl.pre);
    double* part = (double*)((char*)ws + pl.part);
    float* buf[2] = {(float*)((char*)ws + pl.buf), (float*)((char*)ws + pl.buf + pl.buf_bytes)};
    MSMC_LAUNCH(kpp_first_kernel, dim3(1), dim3(64), 0, st, state, (int)first);
    for (int i = 0; i < K; ++i) {
        const int Lcur = i == 0 ? 1 : L, Lnext = i + 1 < K ? L : 0;
        float* cur = buf[i & 1];
        const int rc = kpp_launch_dist(x, state, i == 0 ? nullptr : buf[(i - 1) & 1], cur, part, N, d, pl.T, Lcur, st);
        if (rc) return rc;
        MSMC_LAUNCH(kpp_select_kernel, dim3(1), dim3(256), 0, st, x, part, pre, cur, Lnext ? u + (size_t)i * L : nullptr, state,
                    centers, chosen, potential, N, d, pl.T, Lcur, Lnext, i);
    }
    return msmc_check_launch();
}

}  // extern "C"
