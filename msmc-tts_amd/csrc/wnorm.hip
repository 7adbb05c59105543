// wnorm.hip -- multi-tensor weight norm (forward / backward), bias-gradient column sums, reflect-padding fold and
// leaky-ReLU backward for gfx950: the element-wise and reduction kernels around the convolutions (conv.hip, conv_wgrad.hip).
#include <msmc_rt.hpp>
#include <msmc_hip.h>
#include <msmc_hip_debug.h>
#include "conv_common.inc"

// ================================================================================================
// weight norm (multi-tensor) and bias gradient
// ================================================================================================
MSMC_DEV int wn_find(const msmc_wn_item* items, int n, int blk) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        int mid = (lo + hi + 1) >> 1;
        if (items[mid].block0 <= blk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// sum over the 256 work-items of a workgroup: wave reduction by lane exchange, then four partial sums through LDS
MSMC_DEV float block_sum_fast(float v, float* red4) {
    v = wave_xor_sum(v);
    const int w = threadIdx.x >> 6;
    __syncthreads();                                   // (red4 may still be read from a previous call)
    if ((threadIdx.x & 63) == 0) red4[w] = v;
    __syncthreads();
    return (red4[0] + red4[1]) + (red4[2] + red4[3]);
}

// the same for workgroups of one to four waves (blockDim.x / 64)
MSMC_DEV float block_sum_waves(float v, float* red4) {
    v = wave_xor_sum(v);
    const int w = threadIdx.x >> 6, nw = (int)blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red4[w] = v;
    __syncthreads();
    float s = red4[0];
    for (int q = 1; q < nw; ++q) s = s + red4[q];
    return s;
}

// Row pass: one workgroup per normalised row a (n = Bc * T parameters, contiguous).  The row is read once in its own
// order (sum of squares), then written to layout 1 TAP-OUTER: for a fixed tap the Bc elements of the row are consecutive
// in layout 1 (s1[2] = 1 for every layer the banks build), so a wave stores 64 consecutive elements; the strided re-read
// of the row hits L1.  No per-element integer division (the previous form spent ~60 instructions per parameter on it).
__global__ __launch_bounds__(256) void wn_prepare_kernel(const msmc_wn_item* __restrict__ items, int nitems, int skip2) {
    __shared__ float red[4];
    const msmc_wn_item it = items[wn_find(items, nitems, blockIdx.x)];
    const int a = blockIdx.x - it.block0;
    const int n = it.Bc * it.T, T = it.T, Bc = it.Bc;
    const float* v = it.v + (size_t)a * n;
    float scale = 1.f;
    if (it.g) {                                        // weight norm; g == NULL: plain weight, layout conversion only
        float ss = 0.f;
        if ((n & 3) == 0) {
            const f32x4* v4 = (const f32x4*)v;         // (rows of 4k floats off a 16-byte aligned parameter)
            for (int e = threadIdx.x; e < (n >> 2); e += 256) {
                const f32x4 q = v4[e];
                ss = fmaf(q[0], q[0], ss);
                ss = fmaf(q[1], q[1], ss);
                ss = fmaf(q[2], q[2], ss);
                ss = fmaf(q[3], q[3], ss);
            }
        } else {
            for (int e = threadIdx.x; e < n; e += 256) ss = fmaf(v[e], v[e], ss);
        }
        ss = block_sum_fast(ss, red);
        const float norm = sqrtf(ss);
        scale = it.g[a] / norm;
        if (threadIdx.x == 0) it.inv_norm[a] = 1.f / norm;
    }
    const bool two = it.dst2 && !skip2;
    // (restrict-qualified locals: without them every load of v has to stay behind the previous store to the layout buffers
    //  -- the compiler cannot know they do not overlap -- and the loop runs one memory round trip per element)
    const float* __restrict__ vr = v;
    if (it.dtype == 0) {
        float* __restrict__ d1 = (float*)it.dst1;
        float* __restrict__ d2 = (float*)it.dst2;
        for (int t = 0; t < T; ++t) {
            const long o1 = t * it.s1[0] + a * it.s1[1], o2 = t * it.s2[0] + a * it.s2[1];
            for (int b = threadIdx.x; b < Bc; b += 256) {
                const float wv = vr[b * T + t] * scale;
                d1[o1 + b * it.s1[2]] = wv;
                if (two) d2[o2 + b * it.s2[2]] = wv;
            }
        }
    } else {
        unsigned short* __restrict__ d1 = (unsigned short*)it.dst1;
        unsigned short* __restrict__ d2 = (unsigned short*)it.dst2;
        for (int t = 0; t < T; ++t) {
            const long o1 = t * it.s1[0] + a * it.s1[1], o2 = t * it.s2[0] + a * it.s2[1];
            for (int b = threadIdx.x; b < Bc; b += 256) {
                const unsigned short wv = f32_to_bf16_bits(vr[b * T + t] * scale);
                d1[o1 + b * it.s1[2]] = wv;
                if (two) d2[o2 + b * it.s2[2]] = wv;
            }
        }
    }
}

// Layout 2 is the transpose of the parameter's own order (the normalised axis a runs fastest): written row by row from
// wn_prepare_kernel it is one 2-byte store per cache line.  Here a workgroup owns a tile of 64 rows (a) x 16 columns (b),
// all taps: the parameter is read in its own order (contiguous 16*T floats per row) into LDS and written out with a
// fastest -- 64 consecutive elements per store.  Runs after wn_prepare_kernel (inv_norm); item i owns tile-blocks
// [tblock0, tblock0 + ceil(A/64) * ceil(Bc/16)).  Index walks are incremental (no per-element division).
#define WN_TA 64
#define WN_TB 16
MSMC_DEV int wn_find_tile(const msmc_wn_item* items, int n, int blk) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        int mid = (lo + hi + 1) >> 1;
        if (items[mid].tblock0 <= blk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

#define WN_TC 128                                      // columns (b, t) of a tile staged at once: 33 KB of LDS, four workgroups per CU
__global__ __launch_bounds__(256) void wn_transpose_kernel(const msmc_wn_item* __restrict__ items, int nitems) {
    __shared__ float tile[WN_TA * (WN_TC + 1)];
    __shared__ float scl[WN_TA];
    const msmc_wn_item it = items[wn_find_tile(items, nitems, blockIdx.x)];
    const int tb = blockIdx.x - it.tblock0;
    const int nbt = (it.Bc + WN_TB - 1) / WN_TB;
    const int a0 = (tb / nbt) * WN_TA, b0 = (tb - (tb / nbt) * nbt) * WN_TB;
    const int T = it.T, pitch = WN_TC + 1;
    const int nb = it.Bc - b0 < WN_TB ? it.Bc - b0 : WN_TB, na = it.A - a0 < WN_TA ? it.A - a0 : WN_TA;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ncol = nb * T;
    if (threadIdx.x < WN_TA)
        scl[threadIdx.x] = (it.g && (int)threadIdx.x < na) ? it.g[a0 + threadIdx.x] * it.inv_norm[a0 + threadIdx.x] : 1.f;
    int b = 0, t = w;                                  // column c = b * T + t of this wave's next store
    while (t >= T) { t -= T; ++b; }
    for (int c0 = 0; c0 < ncol; c0 += WN_TC) {
        const int nc = ncol - c0 < WN_TC ? ncol - c0 : WN_TC;
        __syncthreads();                               // (previous chunk's reads done; scl visible)
        for (int r = w; r < na; r += 4) {              // a wave reads nc consecutive floats of one row
            const float* src = it.v + ((size_t)(a0 + r) * it.Bc + b0) * T + c0;
            for (int c = lane; c < nc; c += 64) tile[r * pitch + c] = src[c];
        }
        __syncthreads();
        // lane = row: 64 consecutive a per store; wave w takes columns w, w + 4, .. of the chunk (WN_TC % 4 == 0, so
        // the walk of (b, t) carries over from chunk to chunk)
        const float sc = lane < na ? scl[lane] : 0.f;
        for (int c = w; c < nc; c += 4) {
            if (lane < na)
                el_st_rt(it.dst2, it.dtype, t * it.s2[0] + (a0 + lane) * it.s2[1] + (b0 + b) * it.s2[2], tile[lane * pitch + c] * sc);
            t += 4;
            while (t >= T) { t -= T; ++b; }
        }
    }
}

// Norms of the weight-normalised rows alone (msmc_wn_prepare_multi_tiles): block k takes row norm_rows[k] (an index into the
// grid of ALL rows, as block0 counts them) of item row_item[that row] -- two dependent loads where the binary search over the
// items' block0 was eight, a search that cost each of the 16 000 row workgroups of the autoencoder ~4 us before its first load.
__global__ __launch_bounds__(256) void wn_norm_kernel(const msmc_wn_item* __restrict__ items, const int* __restrict__ row_item,
                                                      const int* __restrict__ norm_rows) {
    __shared__ float red[4];
    const int grow = norm_rows[blockIdx.x];
    const msmc_wn_item it = items[row_item[grow]];
    const int a = grow - it.block0;
    const int n = it.Bc * it.T;
    const float* v = it.v + (size_t)a * n;
    float ss = 0.f;
    if ((n & 3) == 0) {
        const f32x4* v4 = (const f32x4*)v;
        for (int e = threadIdx.x; e < (n >> 2); e += 256) {
            const f32x4 q = v4[e];
            ss = fmaf(q[0], q[0], ss);
            ss = fmaf(q[1], q[1], ss);
            ss = fmaf(q[2], q[2], ss);
            ss = fmaf(q[3], q[3], ss);
        }
    } else {
        for (int e = threadIdx.x; e < n; e += 256) ss = fmaf(v[e], v[e], ss);
    }
    ss = block_sum_fast(ss, red);
    if (threadIdx.x == 0) it.inv_norm[a] = 1.f / sqrtf(ss);
}

// Both kernel layouts from ONE read of the parameter (round 6).  The row pass + transposing pass above moved the autoencoder's
// 36.7 M weights in 91 + 138 us per step -- three reads of v, a workgroup per row, 16 of a wave's 64 lanes loading in the
// transposing pass of every one-tap layer -- for 8 bytes per weight of real traffic, alone on the chip at the head of the step
// (profiles/r06_step_timeline_*.txt).  Here a workgroup owns a tile of TA rows (a) x TB columns (b) x all T taps, TA / TB chosen
// from T so that a row's share of the tile is ~128 contiguous floats or more: the tile is read in the parameter's own order
// (coalesced, whole wave) into LDS and written twice -- layout 2 with a fastest (TA consecutive elements per store), layout 1
// with b fastest (TB consecutive per store; both banks' layouts have s1[2] == 1 and s2[1] == 1, checked by the launcher's
// caller).  The scale g / ||v|| of weight-normalised rows comes from a norms-only row pass in front (wn_norm_kernel).
MSMC_DEV_INLINE int wn_tile_a(int T) { return T <= 4 ? 64 : 32; }
MSMC_DEV_INLINE int wn_tile_b(int T) { return T == 1 ? 128 : T == 2 ? 64 : 32; }
__global__ __launch_bounds__(256) void wn_layout_kernel(const msmc_wn_item* __restrict__ items, int nitems,
                                                        const int* __restrict__ tile_item) {
    MSMC_DYN_LDS(smem);
    float* tile = (float*)smem;
    __shared__ float scl[64];
    const msmc_wn_item it = items[tile_item ? tile_item[blockIdx.x] : wn_find_tile(items, nitems, blockIdx.x)];
    const int T = it.T, TA = wn_tile_a(T), TB = wn_tile_b(T);
    const int tb = blockIdx.x - it.tblock0;
    const int nbt = (it.Bc + TB - 1) / TB;
    const int ti = tb / nbt;
    const int a0 = ti * TA, b0 = (tb - ti * nbt) * TB;
    const int nb = it.Bc - b0 < TB ? it.Bc - b0 : TB, na = it.A - a0 < TA ? it.A - a0 : TA;
    const int ncol = nb * T, pitch = TB * T + 1;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if ((int)threadIdx.x < TA)
        scl[threadIdx.x] = (it.g && (int)threadIdx.x < na) ? it.g[a0 + threadIdx.x] * it.inv_norm[a0 + threadIdx.x] : 1.f;
    {
        // a wave reads rows w, w + 4, .. of the tile, 64 consecutive floats per load; SIXTEEN loads are issued before the first
        // of them is written to LDS (one in flight per work-item made the tile a chain of memory round trips)
        const float* __restrict__ vb = it.v + ((size_t)a0 * it.Bc + b0) * T;
        const size_t rowlen = (size_t)it.Bc * T;
        const int n_k = (ncol + 63) >> 6;
        const int nr = na > w ? (na - w + 3) >> 2 : 0;
        const int P = nr * n_k;
        for (int q0 = 0; q0 < P; q0 += 16) {
            float buf[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int q = q0 + i;
                buf[i] = 0.f;
                if (q < P) {
                    const int j = q / n_k, c = lane + 64 * (q - j * n_k);
                    if (c < ncol) buf[i] = vb[(size_t)(w + 4 * j) * rowlen + c];
                }
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int q = q0 + i;
                if (q < P) {
                    const int j = q / n_k, c = lane + 64 * (q - j * n_k);
                    if (c < ncol) tile[(w + 4 * j) * pitch + c] = buf[i];
                }
            }
        }
    }
    __syncthreads();
    // Stores: FOUR consecutive elements per lane (8 bytes of bf16, 16 of fp32) wherever the fastest axis of a layout is a
    // multiple of four -- a wave instruction of 2-byte stores is 64 separate write requests to the memory pipeline whatever
    // their addresses (the first version of this kernel, one element per lane, moved 1.3 TB/s: no faster than the two
    // passes it replaces); single elements otherwise (the one- and two-channel first layers of the discriminators).
    if (it.dst2) {
        if ((it.A & 3) == 0) {
            // layout 2, a fastest: a lane takes rows 4l .. 4l+3 of one column (b, t); TA / 4 lanes per column
            const int lpc = TA >> 2, cpw = 64 / lpc, csub = lane / lpc, al = (lane - csub * lpc) * 4;
            const int step = 4 * cpw, qs = step / T, rs = step - qs * T;
            int c = w * cpw + csub;
            int b = c / T, t = c - b * T;
            const bool live = al < na;                 // (na is a multiple of four here)
            const float s0 = live ? scl[al] : 0.f, s1_ = live ? scl[al + 1] : 0.f, s2_ = live ? scl[al + 2] : 0.f,
                        s3 = live ? scl[al + 3] : 0.f;
            const float* col = tile + al * pitch;
            for (; c < ncol; c += step) {
                if (live) {
                    const long o = t * it.s2[0] + (a0 + al) + (long)(b0 + b) * it.s2[2];
                    const float x0 = col[c] * s0, x1 = col[pitch + c] * s1_, x2 = col[2 * pitch + c] * s2_, x3 = col[3 * pitch + c] * s3;
                    if (it.dtype == 0) {
                        const f32x4 q = {x0, x1, x2, x3};
                        *(f32x4*)((float*)it.dst2 + o) = q;
                    } else {
                        const u32x2 q = {pack_bf16x2(x0, x1), pack_bf16x2(x2, x3)};
                        *(u32x2*)((unsigned short*)it.dst2 + o) = q;
                    }
                }
                b += qs;
                t += rs;
                if (t >= T) { t -= T; ++b; }
            }
        } else {
            const int cpw = 64 / TA, csub = lane / TA, al = lane - csub * TA;
            const int step = 4 * cpw, qs = step / T, rs = step - qs * T;
            int c = w * cpw + csub;
            int b = c / T, t = c - b * T;
            const float sc = al < na ? scl[al] : 0.f;
            for (; c < ncol; c += step) {
                if (al < na)
                    el_st_rt(it.dst2, it.dtype, t * it.s2[0] + (a0 + al) * it.s2[1] + (b0 + b) * it.s2[2], tile[al * pitch + c] * sc);
                b += qs;
                t += rs;
                if (t >= T) { t -= T; ++b; }
            }
        }
    }
    if ((it.Bc & 3) == 0) {
        // layout 1, b fastest: a lane takes columns 4l .. 4l+3 of one run (a, t); TB / 4 lanes per run
        const int lpr = TB >> 2, rpw = 64 / lpr, sub = lane / lpr, bl = (lane - sub * lpr) * 4;
        const int nrun = na * T;
        for (int run = w * rpw + sub; run < nrun; run += 4 * rpw) {
            if (bl >= nb) continue;                    // (nb is a multiple of four here)
            const int a = run / T, t = run - a * T;
            const float sc = scl[a];
            const long o = t * it.s1[0] + (a0 + a) * it.s1[1] + (b0 + bl);
            const float* row = tile + a * pitch + t + bl * T;
            const float x0 = row[0] * sc, x1 = row[T] * sc, x2 = row[2 * T] * sc, x3 = row[3 * T] * sc;
            if (it.dtype == 0) {
                const f32x4 q = {x0, x1, x2, x3};
                *(f32x4*)((float*)it.dst1 + o) = q;
            } else {
                const u32x2 q = {pack_bf16x2(x0, x1), pack_bf16x2(x2, x3)};
                *(u32x2*)((unsigned short*)it.dst1 + o) = q;
            }
        }
    } else {
        const int lpr = TB < 64 ? TB : 64, rpw = 64 / lpr, sub = lane / lpr, bl = lane - sub * lpr;
        const int nrun = na * T;
        for (int run = w * rpw + sub; run < nrun; run += 4 * rpw) {
            const int a = run / T, t = run - a * T;
            const float sc = scl[a];
            const long o = t * it.s1[0] + (a0 + a) * it.s1[1] + (long)b0 * it.s1[2];
            const float* row = tile + a * pitch + t;
            for (int bb = bl; bb < nb; bb += lpr) el_st_rt(it.dst1, it.dtype, o + bb * it.s1[2], row[bb * T] * sc);
        }
    }
}

// Row pass of the backward: dW arrives in layout 1 (tap-major), v / gv live in the parameter's own order.  Rows of up
// to WN_ROW_MAX parameters go through LDS: dW is read TAP-OUTER (64 consecutive floats per wave load, privatised copies
// folded and zeroed on the way), then everything else runs in the parameter's order (coalesced v reads, coalesced gv
// stores).  Longer rows keep the direct form.
// (Round 4, measured and reverted: all of a row's dW / v loads issued up front from fully unrolled 24-step register arrays
//  -- 77 -> 120 us per call: the predicated steps of short rows and the register footprint cost more than the loads in flight
//  gain; profiles/README.md.  What the loops needed is below: no store between two loads of one array.)
#define WN_ROW_MAX 6144
// NT work-items per row (blockDim.x: 256, or 128 when every row of the bank fits ``row_cap`` <= 4096 floats -- the pass is a chain
// of four memory round trips per row, so its speed is the number of rows in flight per CU: 6 at 256 work-items and a 24 KB row
// buffer, up to 16 at 128 work-items and a buffer sized to the bank's longest row)
__global__ __launch_bounds__(256) void wn_backward_kernel(const msmc_wn_item* __restrict__ items, int nitems,
                                                         int accumulate, int row_cap) {
    MSMC_DYN_LDS(smem);
    float* red = (float*)smem;                         // [4]
    float* row = red + 4;                              // [row_cap]
    const int NT = (int)blockDim.x;
    const msmc_wn_item it = items[wn_find(items, nitems, blockIdx.x)];
    const int a = blockIdx.x - it.block0;
    const int n = it.Bc * it.T, T = it.T, Bc = it.Bc;
    const float* v = it.v + (size_t)a * n;
    float* dw = (float*)it.dw;
    const int R = it.copies > 1 ? it.copies : 1;
    const bool staged = n <= row_cap;
    float dot = 0.f;
    if (staged) {
        // LOADS ONLY in this loop: the accumulators are zeroed in a pass of their own at the end.  With `dw[o] = 0` between two
        // loads of the same array the compiler must keep every load behind the previous store (it cannot prove o' != o), so the
        // loop ran one memory round trip per element: SQ_WAIT_ANY 89 % of the wave cycles, 18 % of the HBM roofline (round 4).
        const float* __restrict__ dwr = dw;
        // (the loads of four steps go out together: one memory round trip per four elements of a work-item instead of one per
        //  element -- the loop bounds are run-time values, so the compiler does not do this on its own)
        if (R == 1) {
            const int nb = (Bc + NT - 1) / NT, steps = T * nb;           // step s: tap s / nb, channel threadIdx.x + NT * (s % nb)
            for (int s0 = 0; s0 < steps; s0 += 4) {
                float q[4];
                int dst[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int s = s0 + u, t = s / nb, b = threadIdx.x + NT * (s - t * nb);
                    const bool ok = s < steps && b < Bc;
                    dst[u] = ok ? b * T + t : -1;
                    q[u] = ok ? dwr[t * it.s1[0] + a * it.s1[1] + b * it.s1[2]] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (dst[u] >= 0) row[dst[u]] = q[u];
            }
        } else if (R <= 8) {
            // privatised copies (the thin layers: eight accumulators per element): all copies of an element requested together,
            // folded in copy order
            for (int t = 0; t < T; ++t) {
                const long o1 = t * it.s1[0] + a * it.s1[1];
                for (int b = threadIdx.x; b < Bc; b += NT) {
                    const long o = o1 + b * it.s1[2];
                    float q[8];
#pragma unroll
                    for (int r = 0; r < 8; ++r) q[r] = r < R ? dwr[o + r * it.dw_copy_stride] : 0.f;
                    float sum = q[0];
#pragma unroll
                    for (int r = 1; r < 8; ++r)
                        if (r < R) sum = sum + q[r];
                    row[b * T + t] = sum;
                }
            }
        } else {
            for (int t = 0; t < T; ++t) {
                const long o1 = t * it.s1[0] + a * it.s1[1];
                for (int b = threadIdx.x; b < Bc; b += NT) {
                    const long o = o1 + b * it.s1[2];
                    float sum = dwr[o];
                    for (int r = 1; r < R; ++r) sum = sum + dwr[o + r * it.dw_copy_stride];      // privatised copies: fold
                    row[b * T + t] = sum;
                }
            }
        }
        __syncthreads();
        if (it.g) {
            const float* __restrict__ vd = v;
            int e = threadIdx.x;
            for (; e + 3 * NT < n; e += 4 * NT) {
                const float v0 = vd[e], v1 = vd[e + NT], v2 = vd[e + 2 * NT], v3 = vd[e + 3 * NT];
                dot = fmaf(row[e], v0, dot);
                dot = fmaf(row[e + NT], v1, dot);
                dot = fmaf(row[e + 2 * NT], v2, dot);
                dot = fmaf(row[e + 3 * NT], v3, dot);
            }
            for (; e < n; e += NT) dot = fmaf(row[e], vd[e], dot);
        }
    } else {
        int b = 0, t = threadIdx.x;
        while (t >= T) { t -= T; ++b; }
        const int db_ = NT / T, dt_ = NT - db_ * T;    // e += NT as (b, t) += (db_, dt_) with carry
        for (int e = threadIdx.x; e < n; e += NT) {
            const long o = t * it.s1[0] + a * it.s1[1] + b * it.s1[2];
            float sum = dw[o];
            for (int r = 1; r < R; ++r) {
                sum = sum + dw[o + r * it.dw_copy_stride];
                dw[o + r * it.dw_copy_stride] = 0.f;
            }
            if (R > 1) dw[o] = sum;
            dot = fmaf(sum, v[e], dot);
            b += db_;
            t += dt_;
            if (t >= T) { t -= T; ++b; }
        }
    }
    float k1 = 1.f, k2 = 0.f;                          // plain weight: gv = dW
    if (it.g) {
        dot = block_sum_waves(dot, red);
        const float inv = it.inv_norm[a], gval = it.g[a];
        if (threadIdx.x == 0) it.gg[a] = accumulate ? it.gg[a] + dot * inv : dot * inv;
        k1 = gval * inv;
        k2 = dot * inv * inv;
    }
    float* gv = it.gv + (size_t)a * n;
    if (staged) {
        const float* __restrict__ vr = v;                  // (v is never written here: its loads may run ahead of the gv stores)
        float* __restrict__ gvr = gv;
        if (accumulate) {
            for (int e = threadIdx.x; e < n; e += NT) gvr[e] = gvr[e] + k1 * (row[e] - vr[e] * k2);
        } else {
            int e = threadIdx.x;
            for (; e + 3 * NT < n; e += 4 * NT) {             // (v was just read by the dot pass: these are cache hits, issued together)
                const float v0 = vr[e], v1 = vr[e + NT], v2 = vr[e + 2 * NT], v3 = vr[e + 3 * NT];
                gvr[e] = k1 * (row[e] - v0 * k2);
                gvr[e + NT] = k1 * (row[e + NT] - v1 * k2);
                gvr[e + 2 * NT] = k1 * (row[e + 2 * NT] - v2 * k2);
                gvr[e + 3 * NT] = k1 * (row[e + 3 * NT] - v3 * k2);
            }
            for (; e < n; e += NT) gvr[e] = k1 * (row[e] - vr[e] * k2);
        }
        for (int t = 0; t < T; ++t) {                      // each accumulator element has exactly this one reader: leave zeros
            const long o1 = t * it.s1[0] + a * it.s1[1];
            for (int b = threadIdx.x; b < Bc; b += NT) {
                const long o = o1 + b * it.s1[2];
                for (int r = 0; r < R; ++r) dw[o + r * it.dw_copy_stride] = 0.f;
            }
        }
    } else {
        int b = 0, t = threadIdx.x;
        while (t >= T) { t -= T; ++b; }
        const int db_ = NT / T, dt_ = NT - db_ * T;
        for (int e = threadIdx.x; e < n; e += NT) {
            const long o = t * it.s1[0] + a * it.s1[1] + b * it.s1[2];
            const float gnew = k1 * (dw[o] - v[e] * k2);
            gv[e] = accumulate ? gv[e] + gnew : gnew;
            dw[o] = 0.f;
            b += db_;
            t += dt_;
            if (t >= T) { t -= T; ++b; }
        }
    }
    if (it.db && threadIdx.x == 0)
        for (int c = a; c < it.nbias; c += it.A) {
            float sum;
            if (R <= 8) {                           // (all copies requested together, folded in copy order: one round trip, not R)
                const float* __restrict__ dbr = it.db;
                float q[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) q[r] = r < R ? dbr[c + r * it.db_copy_stride] : 0.f;
                sum = q[0];
#pragma unroll
                for (int r = 1; r < 8; ++r)
                    if (r < R) sum = sum + q[r];
                for (int r = 0; r < R; ++r) it.db[c + r * it.db_copy_stride] = 0.f;
            } else {
                sum = it.db[c];
                it.db[c] = 0.f;
                for (int r = 1; r < R; ++r) {
                    sum = sum + it.db[c + r * it.db_copy_stride];
                    it.db[c + r * it.db_copy_stride] = 0.f;
                }
            }
            it.gb[c] = accumulate ? it.gb[c] + sum : sum;
        }
}

template <typename T>
__global__ __launch_bounds__(256) void lrelu_bwd_kernel(const T* __restrict__ g, const T* __restrict__ y,
                                                       T* __restrict__ gx, long n, float slope) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
        const float gv = Elt<T>::ld(g + e);
        Elt<T>::st(gx + e, Elt<T>::ld(y + e) > 0.f ? gv : gv * slope);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void colsum_kernel(const T* __restrict__ g, float* __restrict__ out, long rows, int C,
                                                    int rows_per_block) {
    __shared__ float red[256];
    const long r0 = (long)blockIdx.x * rows_per_block;
    long r1 = r0 + rows_per_block;
    if (r1 > rows) r1 = rows;
    const int tid = threadIdx.x;
    if (C >= 256 || (256 % C) != 0) {               // one or more whole columns per work-item
        for (int c = tid; c < C; c += 256) {
            float s = 0.f;
            for (long r = r0; r < r1; ++r) s = s + Elt<T>::ld(g + r * C + c);
            atomicAdd(out + c, s);
        }
        return;
    }
    // C divides 256: the flat index e = tid + 256*k always lands on column tid % C
    const long n = (r1 - r0) * C;
    const T* base = g + r0 * C;
    float s = 0.f;
    for (long e = tid; e < n; e += 256) s = s + Elt<T>::ld(base + e);
    red[tid] = s;
    __syncthreads();
    for (int st = 128; st >= C; st >>= 1) {
        if (tid < st) red[tid] = red[tid] + red[tid + st];
        __syncthreads();
    }
    if (tid < C) atomicAdd(out + tid, red[tid]);
}

// Column sums without atomics (the bias gradients of the transposed convolutions: 10^4 - 10^5 rows of 32-256 channels; the
// atomic form above serialises several hundred same-address atomics per column: 38 us for 12 MB): a block sums a contiguous
// range of rows into part[block][C]; colsum_final_kernel adds the blocks in order (bit-reproducible) into out (+=).
template <typename T>
__global__ __launch_bounds__(256) void colsum_part_kernel(const T* __restrict__ g, float* __restrict__ part, long rows, int C,
                                                         int rows_per_block) {
    __shared__ float red[256 * 8];
    const long r0 = (long)blockIdx.x * rows_per_block;
    long r1 = r0 + rows_per_block;
    if (r1 > rows) r1 = rows;
    const int tid = threadIdx.x;
    float* dst = part + (size_t)blockIdx.x * C;
    constexpr int VE = 16 / (int)sizeof(T);          // elements per 16-byte vector
    if (C % VE == 0 && (256 * VE) % C == 0 && ((size_t)g & 15) == 0) {
        // vector v = tid + 256 k of the block's flat element range always covers the VE columns (tid * VE) % C ..: one
        // 16-byte load per step, VE running sums per work-item, then the work-items of a column group are added in order
        const long nvec = (r1 > r0 ? (r1 - r0) : 0) * C / VE;
        const T* base = g + r0 * C;
        float acc[VE];
#pragma unroll
        for (int q = 0; q < VE; ++q) acc[q] = 0.f;
        for (long v = tid; v < nvec; v += 256) {
            const u32x4 w = *(const u32x4*)(base + v * VE);
#pragma unroll
            for (int q = 0; q < VE; ++q) {
                float x;
                if (sizeof(T) == 4) x = __uint_as_float(w[q & 3]);
                else x = bf16_bits_to_f32((unsigned short)(w[(q >> 1) & 3] >> (16 * (q & 1))));
                acc[q] = acc[q] + x;
            }
        }
#pragma unroll
        for (int q = 0; q < VE; ++q) red[tid * VE + q] = acc[q];
        __syncthreads();
        const int groups = C / VE;                    // work-items t with t % groups == c / VE hold column c at slot c % VE
        for (int c = tid; c < C; c += 256) {
            float s = 0.f;
            for (int t = c / VE; t < 256; t += groups) s = s + red[t * VE + (c % VE)];
            dst[c] = s;
        }
        return;
    }
    if (C >= 256 || (256 % C) != 0) {               // one or more whole columns per work-item
        for (int c = tid; c < C; c += 256) {
            float s = 0.f;
            for (long r = r0; r < r1; ++r) s = s + Elt<T>::ld(g + r * C + c);
            dst[c] = s;
        }
        return;
    }
    const long n = (r1 - r0) * C;                   // C divides 256: the flat index tid + 256 k stays on column tid % C
    const T* base = g + r0 * C;
    float s = 0.f;
    for (long e = tid; e < n; e += 256) s = s + Elt<T>::ld(base + e);
    red[tid] = s;
    __syncthreads();
    for (int st = 128; st >= C; st >>= 1) {
        if (tid < st) red[tid] = red[tid] + red[tid + st];
        __syncthreads();
    }
    if (tid < C) dst[tid] = red[tid];
}
__global__ __launch_bounds__(256) void colsum_final_kernel(const float* __restrict__ part, int nblocks, int C,
                                                           float* __restrict__ out, int accumulate) {
    __shared__ float red[256];
    // 256 / CG slices of blocks per column group of CG = min(C, 256) columns, each summed in order, then added in order
    const int CG = C < 256 ? C : 256, slices = 256 / CG;
    for (int c0 = blockIdx.x * CG; c0 < C; c0 += gridDim.x * CG) {
        const int c = c0 + (int)(threadIdx.x % CG), sl = threadIdx.x / CG;
        const int per = (nblocks + slices - 1) / slices, b0 = sl * per, b1 = b0 + per < nblocks ? b0 + per : nblocks;
        // four interleaved accumulators, combined in a fixed order: the loads of a slice are independent of each other (a single
        // running sum made them one L2 round trip each: 32 us for 512 partial rows)
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        if (sl < slices && c < C) {
            int b = b0;
            for (; b + 4 <= b1; b += 4) {
                s0 = s0 + part[(size_t)b * C + c];
                s1 = s1 + part[(size_t)(b + 1) * C + c];
                s2 = s2 + part[(size_t)(b + 2) * C + c];
                s3 = s3 + part[(size_t)(b + 3) * C + c];
            }
            for (; b < b1; ++b) s0 = s0 + part[(size_t)b * C + c];
        }
        const float s = (s0 + s1) + (s2 + s3);
        __syncthreads();
        red[threadIdx.x] = s;
        __syncthreads();
        if (sl == 0 && c < C) {
            float t = red[threadIdx.x];
            for (int q = 1; q < slices; ++q) t = t + red[q * CG + threadIdx.x];
            out[c] = accumulate ? out[c] + t : t;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void reflect_fold_kernel(const T* __restrict__ gp, const T* __restrict__ mask,
                                                          T* __restrict__ gx, int B, int H, int W, int C, int p,
                                                          float slope, long total) {
    const int Hp = H + 2 * p, Wp = W + 2 * p;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int c = (int)(e % C);
        long r = e / C;
        const int x = (int)(r % W);
        r /= W;
        const int y = (int)(r % H);
        const int b = (int)(r / H);
        // padded rows that reflect onto y: y + p, plus p - y (top border) and 2(H-1) - y + p (bottom border)
        int ys[3], xs[3], ny = 0, nx = 0;
        ys[ny++] = y + p;
        if (y >= 1 && y <= p) ys[ny++] = p - y;
        if (y <= H - 2 && y >= H - 1 - p) ys[ny++] = 2 * (H - 1) - y + p;
        xs[nx++] = x + p;
        if (x >= 1 && x <= p) xs[nx++] = p - x;
        if (x <= W - 2 && x >= W - 1 - p) xs[nx++] = 2 * (W - 1) - x + p;
        float s = 0.f;
        for (int a = 0; a < ny; ++a)
            for (int q = 0; q < nx; ++q) s = s + Elt<T>::ld(gp + (((size_t)b * Hp + ys[a]) * Wp + xs[q]) * C + c);
        if (mask) s = s * (Elt<T>::ld(mask + e) > 0.f ? 1.f : slope);
        Elt<T>::st(gx + e, s);
    }
}

// multi-tensor, vectorised versions of the two element-wise backward helpers (one launch for the same layer of all
// resolution sub-discriminators; V consecutive channels per work-item)
struct FoldMultiArgs {
    int n, p;
    float slope;
    int res_first;                      // 1: (fold + res) * mask -- res is the gradient of a second reader of the ACTIVATED map
    int first[MSMC_GROUP_MAX + 1];
    const void* gp[MSMC_GROUP_MAX];
    const void* mask[MSMC_GROUP_MAX];
    const void* res[MSMC_GROUP_MAX];    // NULL, or [B][H][W][C] added after the mask (a second consumer's gradient)
    void* gx[MSMC_GROUP_MAX];
    int H[MSMC_GROUP_MAX], W[MSMC_GROUP_MAX], C[MSMC_GROUP_MAX];
    long items[MSMC_GROUP_MAX];         // B * H * W * (C / V)
};
// V consecutive channels per work-item (V * sizeof(T) = 16, 8, 4 or sizeof(T) bytes: the widest vector every member's channel
// count allows -- the first layers of the resolution stacks have 4 channels, which kept the whole call on 2-byte accesses);
// 32-bit index arithmetic (items < 2^31 is checked by the launcher: the 64-bit divisions cost more than the memory accesses)
template <typename T, int V>
MSMC_DEV void fold_ld(const T* src, float* out) {
    alignas(16) T v[V];
    if (V * sizeof(T) == 16) *(u32x4*)v = *(const u32x4*)src;
    else if (V * sizeof(T) == 8) *(u32x2*)v = *(const u32x2*)src;
    else if (V * sizeof(T) == 4) *(unsigned int*)v = *(const unsigned int*)src;
    else v[0] = src[0];
#pragma unroll
    for (int q = 0; q < V; ++q) out[q] = Elt<T>::ld(&v[q]);
}
template <typename T, int V>
__global__ __launch_bounds__(256) void reflect_fold_multi_kernel(FoldMultiArgs a) {
    const int k = cv_group_member(a.first, a.n);
    const unsigned nb = (unsigned)(a.first[k + 1] - a.first[k]);
    const int p = a.p;
    const int H = a.H[k], W = a.W[k], C = a.C[k], Hp = H + 2 * p, Wp = W + 2 * p;
    const unsigned CV = (unsigned)(C / V), items = (unsigned)a.items[k];
    const T* gp = (const T*)a.gp[k];
    const T* mask = (const T*)a.mask[k];
    const T* res = (const T*)a.res[k];
    T* gx = (T*)a.gx[k];
    for (unsigned e = (unsigned)(blockIdx.x - a.first[k]) * 256u + threadIdx.x; e < items; e += nb * 256u) {
        const unsigned pix = e / CV;
        const int c = (int)(e - pix * CV) * V;
        const unsigned row = pix / (unsigned)W;
        const int x = (int)(pix - row * (unsigned)W);
        const unsigned b = row / (unsigned)H;
        const int y = (int)(row - b * (unsigned)H);
        int ys[3], xs[3], ny = 0, nx = 0;
        ys[ny++] = y + p;
        if (y >= 1 && y <= p) ys[ny++] = p - y;
        if (y <= H - 2 && y >= H - 1 - p) ys[ny++] = 2 * (H - 1) - y + p;
        xs[nx++] = x + p;
        if (x >= 1 && x <= p) xs[nx++] = p - x;
        if (x <= W - 2 && x >= W - 1 - p) xs[nx++] = 2 * (W - 1) - x + p;
        float sacc[V];
#pragma unroll
        for (int q = 0; q < V; ++q) sacc[q] = 0.f;
        for (int i = 0; i < ny; ++i)
            for (int j = 0; j < nx; ++j) {
                float v[V];
                fold_ld<T, V>(gp + (((size_t)b * Hp + ys[i]) * Wp + xs[j]) * C + c, v);
#pragma unroll
                for (int q = 0; q < V; ++q) sacc[q] = sacc[q] + v[q];
            }
        const size_t o = (size_t)pix * C + c;
        float mv[V], rv[V];
        if (mask) fold_ld<T, V>(mask + o, mv);
        if (res) fold_ld<T, V>(res + o, rv);
        alignas(16) T ov[V];
#pragma unroll
        for (int q = 0; q < V; ++q) {
            float sv = sacc[q];
            if (res && a.res_first) sv = sv + rv[q];
            if (mask) sv = sv * (mv[q] > 0.f ? 1.f : a.slope);
            if (res && !a.res_first) sv = sv + rv[q];
            Elt<T>::st(&ov[q], sv);
        }
        if (V * sizeof(T) == 16) *(u32x4*)(gx + o) = *(const u32x4*)ov;
        else if (V * sizeof(T) == 8) *(u32x2*)(gx + o) = *(const u32x2*)ov;
        else if (V * sizeof(T) == 4) *(unsigned int*)(gx + o) = *(const unsigned int*)ov;
        else gx[o] = ov[0];
    }
}

struct LreluMultiArgs {
    int n;
    float slope;
    int first[MSMC_GROUP_MAX + 1];
    const void* g[MSMC_GROUP_MAX];
    const void* y[MSMC_GROUP_MAX];
    void* gx[MSMC_GROUP_MAX];
    long items[MSMC_GROUP_MAX];         // elements / V
};
template <typename T, int V>
__global__ __launch_bounds__(256) void lrelu_bwd_multi_kernel(LreluMultiArgs a) {
    const int k = cv_group_member(a.first, a.n);
    const int nb = a.first[k + 1] - a.first[k];
    const T* g = (const T*)a.g[k];
    const T* y = (const T*)a.y[k];
    T* gx = (T*)a.gx[k];
    for (long e = (long)(blockIdx.x - a.first[k]) * 256 + threadIdx.x; e < a.items[k]; e += (long)nb * 256) {
        alignas(16) T gv[V], yv[V], ov[V];
        if (V * sizeof(T) == 16) {
            *(u32x4*)gv = *(const u32x4*)(g + e * V);
            *(u32x4*)yv = *(const u32x4*)(y + e * V);
        } else {
            gv[0] = g[e];
            yv[0] = y[e];
        }
#pragma unroll
        for (int q = 0; q < V; ++q) {
            const float gf = Elt<T>::ld(&gv[q]);
            Elt<T>::st(&ov[q], Elt<T>::ld(&yv[q]) > 0.f ? gf : gf * a.slope);
        }
        if (V * sizeof(T) == 16) *(u32x4*)(gx + e * V) = *(const u32x4*)ov;
        else gx[e] = ov[0];
    }
}

__global__ void zero_kernel(float* p, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0.f;
}

template <typename T>
static int fold_multi_launch(FoldMultiArgs& a, int v, int blocks, msmc_stream stream) {
    constexpr int VMAX = Elt<T>::VEC;           // 16-byte vectors: 4 fp32 / 8 bf16
    if (v == VMAX) MSMC_LAUNCH((reflect_fold_multi_kernel<T, VMAX>), dim3((unsigned)blocks), dim3(256), 0, (msmc_stream_t)stream, a);
    else if (v == VMAX / 2) MSMC_LAUNCH((reflect_fold_multi_kernel<T, VMAX / 2>), dim3((unsigned)blocks), dim3(256), 0, (msmc_stream_t)stream, a);
    else if (v == 2 && VMAX == 8) MSMC_LAUNCH((reflect_fold_multi_kernel<T, 2>), dim3((unsigned)blocks), dim3(256), 0, (msmc_stream_t)stream, a);
    else MSMC_LAUNCH((reflect_fold_multi_kernel<T, 1>), dim3((unsigned)blocks), dim3(256), 0, (msmc_stream_t)stream, a);
    return msmc_check_launch();
}

template <typename T>
static int lrelu_multi_launch(LreluMultiArgs& a, bool vec, int blocks, msmc_stream stream) {
    if (vec) MSMC_LAUNCH((lrelu_bwd_multi_kernel<T, Elt<T>::VEC>), dim3((unsigned)blocks), dim3(256), 0, (msmc_stream_t)stream, a);
    else MSMC_LAUNCH((lrelu_bwd_multi_kernel<T, 1>), dim3((unsigned)blocks), dim3(256), 0, (msmc_stream_t)stream, a);
    return msmc_check_launch();
}

extern "C" {

int msmc_wn_prepare_multi(const msmc_wn_item* items, int nitems, int total_blocks, msmc_stream stream) {
    if (!items || nitems <= 0 || total_blocks <= 0) return MSMC_E_SHAPE;
    MSMC_LAUNCH(wn_prepare_kernel, dim3(total_blocks), dim3(256), 0, (msmc_stream_t)stream, items, nitems, 0);
    return msmc_check_launch();
}

int msmc_wn_prepare_multi_tiled(const msmc_wn_item* items, int nitems, int total_blocks, int total_tile_blocks,
                                msmc_stream stream) {
    if (!items || nitems <= 0 || total_blocks <= 0 || total_tile_blocks < 0) return MSMC_E_SHAPE;
    MSMC_LAUNCH(wn_prepare_kernel, dim3(total_blocks), dim3(256), 0, (msmc_stream_t)stream, items, nitems, 1);
    int rc = msmc_check_launch();
    if (rc || total_tile_blocks == 0) return rc;
    MSMC_LAUNCH(wn_transpose_kernel, dim3(total_tile_blocks), dim3(256), 0, (msmc_stream_t)stream, items, nitems);
    return msmc_check_launch();
}

// tile-blocks of one item under wn_layout_kernel's tile rule (the host lays tblock0 out with it)
int msmc_wn_tile_blocks(int A, int Bc, int T) {
    if (A <= 0 || Bc <= 0 || T <= 0) return 0;
    const int ta = T <= 4 ? 64 : 32, tb = T == 1 ? 128 : T == 2 ? 64 : 32;
    return ((A + ta - 1) / ta) * ((Bc + tb - 1) / tb);
}
int msmc_wn_prepare_multi_tiles(const msmc_wn_item* items, int nitems, int total_blocks, int total_tile_blocks, int max_taps,
                                const int* row_item, const int* norm_rows, int n_norm_rows, const int* tile_item,
                                msmc_stream stream) {
    if (!items || nitems <= 0 || total_blocks <= 0 || total_tile_blocks <= 0 || max_taps <= 0 || max_taps > MSMC_CONV_MAX_TAPS ||
        n_norm_rows < 0 || (n_norm_rows > 0 && (!row_item || !norm_rows)))
        return MSMC_E_SHAPE;
    if (n_norm_rows > 0) {
        MSMC_LAUNCH(wn_norm_kernel, dim3(n_norm_rows), dim3(256), 0, (msmc_stream_t)stream, items, row_item, norm_rows);
        int rc = msmc_check_launch();
        if (rc) return rc;
    }
    size_t lds = 0;
    for (int T = 1; T <= max_taps; ++T) {
        const int ta = T <= 4 ? 64 : 32, tb = T == 1 ? 128 : T == 2 ? 64 : 32;
        const size_t l = (size_t)ta * (tb * T + 1) * sizeof(float);
        if (l > lds) lds = l;
    }
    int rc = msmc_allow_lds((const void*)wn_layout_kernel, (int)lds);
    if (rc) return rc;
    MSMC_LAUNCH(wn_layout_kernel, dim3(total_tile_blocks), dim3(256), lds, (msmc_stream_t)stream, items, nitems, tile_item);
    return msmc_check_launch();
}

int msmc_wn_backward_multi_rows(const msmc_wn_item* items, int nitems, int total_blocks, int accumulate, int max_row,
                                msmc_stream stream) {
    if (!items || nitems <= 0 || total_blocks <= 0) return MSMC_E_SHAPE;
    // max_row: the longest normalised row (Bc * T parameters) among the items, 0 = unknown.  Rows up to 4096 floats: 128
    // work-items per row and a row buffer of that size (more rows in flight per CU); otherwise the 256 / 24 KB form, whose
    // rows beyond WN_ROW_MAX take the unstaged path
    const bool small = max_row > 0 && max_row <= 4096;
    const int cap = small ? ((max_row + 63) & ~63) : WN_ROW_MAX;
    const size_t lds = 16 + (size_t)cap * sizeof(float);
    int rc = msmc_allow_lds((const void*)wn_backward_kernel, (int)lds);
    if (rc) return rc;
    MSMC_LAUNCH(wn_backward_kernel, dim3(total_blocks), dim3(small ? 128 : 256), lds, (msmc_stream_t)stream, items, nitems,
                accumulate, cap);
    return msmc_check_launch();
}

int msmc_wn_backward_multi_acc(const msmc_wn_item* items, int nitems, int total_blocks, int accumulate, msmc_stream stream) {
    return msmc_wn_backward_multi_rows(items, nitems, total_blocks, accumulate, 0, stream);
}

int msmc_wn_backward_multi(const msmc_wn_item* items, int nitems, int total_blocks, msmc_stream stream) {
    return msmc_wn_backward_multi_acc(items, nitems, total_blocks, 0, stream);
}

int msmc_reflect_fold(const void* gp, const void* mask_src, void* gx, int B, int H, int W, int C, int p, float slope,
                      int dtype, msmc_stream stream) {
    if (!gp || !gx || B <= 0 || H <= p || W <= p || C <= 0 || p < 0) return MSMC_E_SHAPE;
    const long total = (long)B * H * W * C;
    long blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
#define WN_GO(T_)                                                                                                   \
    MSMC_LAUNCH(reflect_fold_kernel<T_>, dim3((unsigned)blocks), dim3(256), 0, (msmc_stream_t)stream, (const T_*)gp,     \
                (const T_*)mask_src, (T_*)gx, B, H, W, C, p, slope, total)
    MSMC_BY_DTYPE(dtype, WN_GO);
#undef WN_GO
    return msmc_check_launch();
}

int msmc_lrelu_bwd(const void* g, const void* y, void* gx, long n, float slope, int dtype, msmc_stream stream) {
    if (!g || !y || !gx || n <= 0) return MSMC_E_SHAPE;
    long blocks = (n + 1023) / 1024;
    if (blocks > 2048) blocks = 2048;
#define WN_GO(T_)                                                                                                   \
    MSMC_LAUNCH(lrelu_bwd_kernel<T_>, dim3((unsigned)blocks), dim3(256), 0, (msmc_stream_t)stream, (const T_*)g,         \
                (const T_*)y, (T_*)gx, n, slope)
    MSMC_BY_DTYPE(dtype, WN_GO);
#undef WN_GO
    return msmc_check_launch();
}

int msmc_reflect_fold_multi(const void* const* gp, const void* const* mask_src, void* const* gx, const int* B, const int* H,
                            const int* W, const int* C, int n, int p, float slope, int dtype, msmc_stream stream) {
    return msmc_reflect_fold_multi_res(gp, mask_src, nullptr, gx, B, H, W, C, n, p, slope, dtype, stream);
}

static int fold_multi_impl(const void* const* gp, const void* const* mask_src, const void* const* res, void* const* gx,
                           const int* B, const int* H, const int* W, const int* C, int n, int p, float slope, int dtype,
                           int res_first, msmc_stream stream);

int msmc_reflect_fold_multi_res(const void* const* gp, const void* const* mask_src, const void* const* res, void* const* gx,
                                const int* B, const int* H, const int* W, const int* C, int n, int p, float slope, int dtype,
                                msmc_stream stream) {
    return fold_multi_impl(gp, mask_src, res, gx, B, H, W, C, n, p, slope, dtype, 0, stream);
}

int msmc_reflect_fold_multi_tap(const void* const* gp, const void* const* mask_src, const void* const* tap, void* const* gx,
                                const int* B, const int* H, const int* W, const int* C, int n, int p, float slope, int dtype,
                                msmc_stream stream) {
    return fold_multi_impl(gp, mask_src, tap, gx, B, H, W, C, n, p, slope, dtype, 1, stream);
}

static int colsum_blocks(long rows) {
    long nb = (rows + 127) / 128;                    // >= 128 rows per block, at most one block per CU (the second stage is ONE
    if (nb > 256) nb = 256;                          // workgroup per 256 columns: it reads nb rows of partial sums)
    return (int)(nb < 1 ? 1 : nb);
}
size_t msmc_colsum_workspace(long rows, int C) { return rows > 0 && C > 0 ? (size_t)colsum_blocks(rows) * C * sizeof(float) : 0; }
int msmc_colsum_ws(const void* g, float* out, long rows, int C, int dtype, int accumulate, void* workspace,
                   size_t workspace_bytes, msmc_stream stream) {
    if (!g || !out || rows <= 0 || C <= 0) return MSMC_E_SHAPE;
    if (!workspace || workspace_bytes < msmc_colsum_workspace(rows, C)) return MSMC_E_WORKSPACE;
    const int nb = colsum_blocks(rows);
    const int rpb = (int)((rows + nb - 1) / nb);
    float* part = (float*)workspace;
#define WN_GO(T_) MSMC_LAUNCH(colsum_part_kernel<T_>, dim3(nb), dim3(256), 0, (msmc_stream_t)stream, (const T_*)g, part, rows, C, rpb)
    MSMC_BY_DTYPE(dtype, WN_GO);
#undef WN_GO
    int rc = msmc_check_launch();
    if (rc) return rc;
    const int used = (int)((rows + rpb - 1) / rpb);  // (blocks that own rows)
    MSMC_LAUNCH(colsum_final_kernel, dim3((C + 255) / 256), dim3(256), 0, (msmc_stream_t)stream, (const float*)part, used, C, out,
                accumulate);
    return msmc_check_launch();
}

}  // extern "C"

static int fold_multi_impl(const void* const* gp, const void* const* mask_src, const void* const* res, void* const* gx,
                           const int* B, const int* H, const int* W, const int* C, int n, int p, float slope, int dtype,
                           int res_first, msmc_stream stream) {
    if (!gp || !gx || !B || !H || !W || !C || n <= 0 || n > MSMC_GROUP_MAX || p < 0 || dtype < 0 || dtype > 1)
        return MSMC_E_SHAPE;
    int v = dtype == 0 ? 4 : 8;                 // widest vector (in elements) every member's channel count is a multiple of
    for (int k = 0; k < n; ++k) {
        if (!gp[k] || !gx[k] || B[k] <= 0 || C[k] <= 0 || H[k] <= p || W[k] <= p) return MSMC_E_SHAPE;
        while (v > 1 && (C[k] % v) != 0) v >>= 1;
    }
    for (int k = 0; k < n; ++k)                 // (16 / 8 / 4-byte accesses need that alignment of every operand)
        while (v > 1 && (((size_t)gp[k] | (size_t)gx[k] | (size_t)(mask_src && mask_src[k] ? mask_src[k] : nullptr) |
                          (size_t)(res && res[k] ? res[k] : nullptr)) & (size_t)(v * (dtype == 0 ? 4 : 2) - 1)))
            v >>= 1;
    FoldMultiArgs a;
    a.n = n;
    a.p = p;
    a.slope = slope;
    a.res_first = res_first;
    int blocks = 0;
    for (int k = 0; k < n; ++k) {
        a.gp[k] = gp[k];
        a.mask[k] = mask_src ? mask_src[k] : nullptr;
        a.res[k] = res ? res[k] : nullptr;
        a.gx[k] = gx[k];
        a.H[k] = H[k];
        a.W[k] = W[k];
        a.C[k] = C[k];
        a.items[k] = (long)B[k] * H[k] * W[k] * (C[k] / v);
        if (a.items[k] >= (1L << 31)) return MSMC_E_SHAPE;
        long nb = (a.items[k] + 255) / 256;
        if (nb > 16L * MSMC_NUM_CU) nb = 16L * MSMC_NUM_CU;       // (one or two items per work-item: an item's loads cannot run ahead of the
        a.first[k] = blocks;                                      //  previous item's store, so parallelism has to come from the grid)
        blocks += (int)(nb < 1 ? 1 : nb);
    }
    a.first[n] = blocks;
    return dtype == 0 ? fold_multi_launch<float>(a, v, blocks, stream) : fold_multi_launch<unsigned short>(a, v, blocks, stream);
}

extern "C" {

int msmc_lrelu_bwd_multi(const void* const* g, const void* const* y, void* const* gx, const long* nelem, int n, float slope,
                         int dtype, msmc_stream stream) {
    if (!g || !y || !gx || !nelem || n <= 0 || n > MSMC_GROUP_MAX || dtype < 0 || dtype > 1) return MSMC_E_SHAPE;
    const int VEC = dtype == 0 ? 4 : 8;
    bool vec = true;
    for (int k = 0; k < n; ++k) {
        if (!g[k] || !y[k] || !gx[k] || nelem[k] <= 0) return MSMC_E_SHAPE;
        // (the 16-byte kernel needs whole vectors and that alignment of every operand: a contiguous view may start anywhere)
        vec = vec && (nelem[k] % VEC) == 0 && (((size_t)g[k] | (size_t)y[k] | (size_t)gx[k]) & 15) == 0;
    }
    LreluMultiArgs a;
    a.n = n;
    a.slope = slope;
    int blocks = 0;
    for (int k = 0; k < n; ++k) {
        a.g[k] = g[k];
        a.y[k] = y[k];
        a.gx[k] = gx[k];
        a.items[k] = nelem[k] / (vec ? VEC : 1);
        long nb = (a.items[k] + 255) / 256;
        if (nb > 4L * MSMC_NUM_CU) nb = 4L * MSMC_NUM_CU;
        a.first[k] = blocks;
        blocks += (int)(nb < 1 ? 1 : nb);
    }
    a.first[n] = blocks;
    return dtype == 0 ? lrelu_multi_launch<float>(a, vec, blocks, stream) : lrelu_multi_launch<unsigned short>(a, vec, blocks, stream);
}

int msmc_colsum(const void* g, float* out, long rows, int C, int dtype, msmc_stream stream) {
    if (!g || !out || rows <= 0 || C <= 0) return MSMC_E_SHAPE;
    MSMC_LAUNCH(zero_kernel, dim3((C + 255) / 256), dim3(256), 0, (msmc_stream_t)stream, out, C);
    int rpb = 256;
    while ((rows + rpb - 1) / rpb > 4096) rpb <<= 1;
    dim3 grid((unsigned)((rows + rpb - 1) / rpb));
#define WN_GO(T_) MSMC_LAUNCH(colsum_kernel<T_>, grid, dim3(256), 0, (msmc_stream_t)stream, (const T_*)g, out, rows, C, rpb)
    MSMC_BY_DTYPE(dtype, WN_GO);
#undef WN_GO
    return msmc_check_launch();
}

}  // extern "C"
