// units.hip -- what follows the labels in a discrete-unit pipeline, for gfx950: collapsing repeated labels into (unit,
// duration) runs (msmc_units_collapse), counting how often every code is used (msmc_units_usage) and the way back from runs to
// frame labels (msmc_units_total, msmc_units_expand).  The labels come from msmc_vq_assign_wide (vq_assign.inc); the host side is
// msmctts_amd/hip/units.py.  Integer work only: every result is exact.
//
// msmc_units_collapse: one workgroup of 256 work-items per utterance walks the valid prefix ind[b][0 .. min(length[b], T)) in
// chunks of 256 frames.  Frame t starts a run when t == 0 or ind[b][t] != ind[b][t - 1]; an exclusive scan of those flags in LDS
// numbers the runs of the chunk, and the run starts of the chunk are left in LDS in run order.  Two values are carried from chunk
// to chunk: the runs so far and the frame at which the current (last) run started -- so a run may span any number of chunks.
// The work-item that starts run r writes units[b][r] and closes run r - 1: dur[b][r - 1] = t - (start of run r - 1); the last
// run is closed against the prefix's end behind the loop.  The slots r >= ulen[b] get units = -1, dur = 0: every element of
// units, dur and ulen is written exactly once, and nothing at or beyond length[b] is read.
//
// msmc_units_expand, the inverse: one workgroup of 256 work-items per utterance walks the runs r < min(max(ulen[b], 0), R) in
// chunks of 256 runs.  An inclusive scan (64-bit) of the chunk's durations max(dur, 0) in LDS gives every run's first frame, the
// chunk's units sit next to them; one value is carried from chunk to chunk: the frames so far.  The work-items then stride over
// the chunk's frames [frames so far, + chunk total) below T -- consecutive work-items, consecutive frames -- and each finds its
// run as the LAST run of the chunk that starts at or before its frame (binary search of the LDS starts): runs of no frames share
// their start with the run behind them and are passed over.  Behind the loop the frames from min(total, T) to T get -1 and
// length[b] = min(total, T): every element of ind and length is written exactly once, nothing at or beyond ulen[b] is read.  The
// walk stops at the first chunk boundary at or beyond T.  msmc_units_total: the same sum alone, one workgroup per utterance.
//
// msmc_units_usage: the frames of all utterances, flattened, are cut into parts of whole 256-frame tiles, one workgroup per
// part.  A workgroup counts its valid frames per code in UN_HIST LDS counters (integer atomics), a pass per UN_HIST codes, and
// adds its non-zero counters onto counts with 64-bit integer atomics: exact, whatever the order.  Without accumulate a first
// launch zeroes counts.  Labels outside [0, K) are skipped.
#include <msmc_rt.hpp>
#include <msmc_hip.h>

#define UN_WG 256            // work-items of a workgroup = frames of a chunk
#define UN_HIST 4096         // LDS counters per histogram pass

__global__ __launch_bounds__(UN_WG) void units_collapse_kernel(const int64_t* __restrict__ ind, const int64_t* __restrict__ length,
                                                              int64_t* __restrict__ units, int32_t* __restrict__ dur,
                                                              int64_t* __restrict__ ulen, int T) {
    __shared__ int sc[UN_WG];            // inclusive scan of the run-start flags of the chunk
    __shared__ int starts[UN_WG];        // frame at which run e of the chunk starts
    const int tid = threadIdx.x;
    const size_t row = (size_t)blockIdx.x * T;
    const int64_t lb = length[blockIdx.x];
    const int len = lb <= 0 ? 0 : (lb < T ? (int)lb : T);
    int runs = 0, cur = 0;               // carried: runs so far, first frame of the last of them
    for (int t0 = 0; t0 < len; t0 += UN_WG) {
        const int t = t0 + tid;
        int64_t v = 0;
        int flag = 0;
        if (t < len) {
            v = ind[row + t];
            flag = (t == 0 || v != ind[row + t - 1]) ? 1 : 0;
        }
        sc[tid] = flag;
        __syncthreads();
        for (int off = 1; off < UN_WG; off <<= 1) {
            const int add = tid >= off ? sc[tid - off] : 0;
            __syncthreads();
            sc[tid] += add;
            __syncthreads();
        }
        const int e = sc[tid] - flag;    // runs of this chunk that start before frame t
        if (flag) starts[e] = t;
        __syncthreads();
        if (flag) {
            const int r = runs + e;
            units[row + r] = v;
            if (r > 0) dur[row + r - 1] = t - (e > 0 ? starts[e - 1] : cur);
        }
        const int n = sc[UN_WG - 1];
        if (n > 0) cur = starts[n - 1];
        runs += n;
        __syncthreads();                 // the next chunk overwrites sc / starts
    }
    if (tid == 0) {
        if (runs > 0) dur[row + runs - 1] = len - cur;
        ulen[blockIdx.x] = runs;
    }
    for (int r = runs + tid; r < T; r += UN_WG) {
        units[row + r] = -1;
        dur[row + r] = 0;
    }
}

MSMC_DEV int un_runs(int64_t ulen, int R) { return ulen <= 0 ? 0 : (ulen < R ? (int)ulen : R); }

__global__ __launch_bounds__(UN_WG) void units_total_kernel(const int32_t* __restrict__ dur, const int64_t* __restrict__ ulen,
                                                           int64_t* __restrict__ total, int R) {
    __shared__ long long part[UN_WG];
    const int tid = threadIdx.x;
    const size_t row = (size_t)blockIdx.x * R;
    const int n = un_runs(ulen[blockIdx.x], R);
    long long s = 0;
    for (int r = tid; r < n; r += UN_WG) {
        const int d = dur[row + r];
        s += d > 0 ? d : 0;
    }
    part[tid] = s;
    __syncthreads();
    for (int off = UN_WG / 2; off > 0; off >>= 1) {
        if (tid < off) part[tid] += part[tid + off];
        __syncthreads();
    }
    if (tid == 0) total[blockIdx.x] = part[0];
}

__global__ __launch_bounds__(UN_WG) void units_expand_kernel(const int64_t* __restrict__ units, const int32_t* __restrict__ dur,
                                                            const int64_t* __restrict__ ulen, int64_t* __restrict__ ind,
                                                            int64_t* __restrict__ length, int R, int T) {
    __shared__ long long sc[UN_WG];      // inclusive scan of the chunk's durations, then the first frame of every run
    __shared__ long long su[UN_WG];      // the chunk's units
    const int tid = threadIdx.x;
    const size_t urow = (size_t)blockIdx.x * R, irow = (size_t)blockIdx.x * T;
    const int n = un_runs(ulen[blockIdx.x], R);
    long long base = 0;                  // carried: frames of the runs before this chunk
    for (int r0 = 0; r0 < n && base < T; r0 += UN_WG) {
        const int r = r0 + tid;
        long long d = 0;
        if (r < n) {
            const int dv = dur[urow + r];
            d = dv > 0 ? dv : 0;
            su[tid] = units[urow + r];
        }
        sc[tid] = d;
        __syncthreads();
        for (int off = 1; off < UN_WG; off <<= 1) {
            const long long add = tid >= off ? sc[tid - off] : 0;
            __syncthreads();
            sc[tid] += add;
            __syncthreads();
        }
        const long long tot = sc[UN_WG - 1];
        const long long mine = base + sc[tid] - d;
        __syncthreads();
        sc[tid] = mine;
        __syncthreads();
        const long long end = base + tot < T ? base + tot : T;
        for (long long t = base + tid; t < end; t += UN_WG) {
            int e = 0, hi = UN_WG;       // the last run of the chunk with sc[e] <= t (sc[0] = base <= t)
            while (hi - e > 1) {
                const int mid = (e + hi) >> 1;
                if (sc[mid] <= t) e = mid;
                else hi = mid;
            }
            ind[irow + t] = su[e];
        }
        base += tot;
        __syncthreads();                 // the next chunk overwrites sc / su
    }
    const int len = base < T ? (int)base : T;
    if (tid == 0) length[blockIdx.x] = len;
    for (int t = len + tid; t < T; t += UN_WG) ind[irow + t] = -1;
}

__global__ __launch_bounds__(256) void units_zero_kernel(int64_t* __restrict__ counts, int K) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k < K) counts[k] = 0;
}

__global__ __launch_bounds__(UN_WG) void units_usage_kernel(const int64_t* __restrict__ ind, const int64_t* __restrict__ length,
                                                           int64_t* counts, long total, int T, int K, long part) {
    __shared__ int h[UN_HIST];
    const int tid = threadIdx.x;
    const long e0 = (long)blockIdx.x * part, e1 = e0 + part < total ? e0 + part : total;
    for (long k0 = 0; k0 < K; k0 += UN_HIST) {              // (K <= 4096: one pass over the part's labels)
        const int kn = K - k0 < UN_HIST ? (int)(K - k0) : UN_HIST;
        for (int i = tid; i < kn; i += UN_WG) h[i] = 0;
        __syncthreads();
        for (long e = e0 + tid; e < e1; e += UN_WG) {
            const long b = e / T;
            if (e - b * T < length[b]) {
                const int64_t v = ind[e];
                if (v >= k0 && v < k0 + kn) atomicAdd(&h[(int)(v - k0)], 1);
            }
        }
        __syncthreads();
        for (int i = tid; i < kn; i += UN_WG) {
            const int c = h[i];
            if (c) atomicAdd((unsigned long long*)(counts + k0 + i), (unsigned long long)c);
        }
        __syncthreads();
    }
}

extern "C" {

int msmc_units_collapse(const int64_t* ind, const int64_t* length, int64_t* units, int32_t* dur, int64_t* ulen, int B, int T,
                        msmc_stream stream) {
    if (B <= 0 || T <= 0) return MSMC_E_SHAPE;
    MSMC_LAUNCH(units_collapse_kernel, dim3((unsigned)B), dim3(UN_WG), 0, (msmc_stream_t)stream, ind, length, units, dur, ulen, T);
    return msmc_check_launch();
}

int msmc_units_total(const int32_t* dur, const int64_t* ulen, int64_t* total, int B, int R, msmc_stream stream) {
    if (B <= 0 || R <= 0) return MSMC_E_SHAPE;
    MSMC_LAUNCH(units_total_kernel, dim3((unsigned)B), dim3(UN_WG), 0, (msmc_stream_t)stream, dur, ulen, total, R);
    return msmc_check_launch();
}

int msmc_units_expand(const int64_t* units, const int32_t* dur, const int64_t* ulen, int64_t* ind, int64_t* length, int B, int R,
                      int T, msmc_stream stream) {
    if (B <= 0 || R <= 0 || T <= 0) return MSMC_E_SHAPE;
    MSMC_LAUNCH(units_expand_kernel, dim3((unsigned)B), dim3(UN_WG), 0, (msmc_stream_t)stream, units, dur, ulen, ind, length, R, T);
    return msmc_check_launch();
}

int msmc_units_usage(const int64_t* ind, const int64_t* length, int64_t* counts, int B, int T, int K, int accumulate,
                     msmc_stream stream) {
    if (B <= 0 || T <= 0 || K <= 0) return MSMC_E_SHAPE;
    msmc_stream_t st = (msmc_stream_t)stream;
    if (!accumulate) MSMC_LAUNCH(units_zero_kernel, dim3((unsigned)((K + 255L) / 256)), dim3(256), 0, st, counts, K);
    // parts of whole tiles: enough frames per workgroup (16 tiles) to pay for its K global adds, at most four workgroups per CU
    const long total = (long)B * T, tiles = (total + UN_WG - 1) / UN_WG;
    long P = (tiles + 15) / 16;
    if (P > 4L * MSMC_NUM_CU) P = 4L * MSMC_NUM_CU;
    const long part = (tiles + P - 1) / P * UN_WG;
    P = (total + part - 1) / part;
    MSMC_LAUNCH(units_usage_kernel, dim3((unsigned)P), dim3(UN_WG), 0, st, ind, length, counts, total, T, K, part);
    return msmc_check_launch();
}

}  // extern "C"
