// side_enc.hip -- the pitch / energy side encoder of MAMSEncoder (reference networks/vqgantts/msmc_vqgan_emb.py:41-120), for
// gfx950: its thin first layer with the Tanh behind it, and the ceil-mode average pooling of the side encoding fused with the
// addition to a stage's output.  Host side: msmctts_amd/hip/side_enc.py (side_front, pool_add).  The three C -> C layers between
// the two run on the implicit-GEMM convolution kernels; those take in_channels % 8 == 0, and the first layer has P + E = 2 input
// channels: 14 multiply-adds per output element, nothing for the matrix cores, bound by the store of y.
//
// ---- msmc_side_front_fwd (sf_fwd_kernel) -------------------------------------------------------------------------------------------
// y[b][t][c] = tanhf(z), z = bias[c] + sum_ci sum_k w[c][ci][k] x[b][t + k - pad][ci], pad = (taps - 1) / 2, x = 0 outside
// [0, T); channel ci < P is pitch[b][t][ci], channel ci >= P is energy[b][t][ci - P]: the two tensors are read where they are, no
// concatenated copy.  No length masking (the reference convolves over the padded frames as well).
// Work split: a workgroup of 256 work-items owns SF_FT = 32 frames of one utterance and all C channels.  It stages the whole
// weight in LDS as wl[(ci taps + k) C + c] (the channel fastest: the eight channels of a work-item are two 16-byte LDS reads,
// consecutive work-items read consecutive addresses), the bias behind it, and the SF_FT + taps - 1 input frames of the tile,
// zero-filled outside the utterance, as xs[frame][ci].  A work-item then computes 8 consecutive channels of one frame at a time
// (piece e = frame (C / 8) + channel group, e = work-item, + 256, ...) and stores them as one 16-byte (bf16) or two 16-byte (fp32)
// accesses.
// ORDER of one output element (restated by tests/_sideenccases.py): acc = bias[c]; for ci = 0 .. Cin - 1, for k = 0 .. taps - 1:
// acc = acc + fl(w[c][ci][k] * x) -- a rounded product and a rounded addition each (the build contracts nothing); y = tanhf(acc),
// the device function msmc_tanh_f32_fwd calls, rounded once more for a bf16 output.
//
// ---- msmc_side_front_bwd (sf_bwd_kernel, sf_bwd_sum_kernel) --------------------------------------------------------------------
// dz[b][t][c] = gy (1 - y y) from y and gy as fp32 (bf16 operands widened exactly): fl(gy * fl(1 - fl(y * y))).
// dw[c][ci][k] = sum_{b,t} dz[b][t][c] x[b][t + k - pad][ci], db[c] = sum_{b,t} dz[b][t][c].  No gradient to pitch / energy.
// Launch 1: a workgroup owns a tile of SF_FT frames of one utterance (tile index = b tiles_per_utterance + tile, the forward's
// tiling) and stages its input frames as the forward does.  A work-item owns one (ci, c) pair at a time (item = ci C + c, the
// channel fastest: the loads of y and gy coalesce) and keeps the taps sums of that pair in registers: for the frames of the
// tile in ascending order, s_k = s_k + fl(dz * xs[frame + k][ci]), each from +0; the work-items with ci == 0 also
// s_b = s_b + dz.  The partials go to the workspace: part[tile][c (Cin taps) + ci taps + k] and, behind the dw part of the tile,
// part[tile][C Cin taps + c].  Launch 2: element e of (dw, db) = (((+0 + part[0][e]) + part[1][e]) + ...) over the tiles in
// ascending index.  No floating-point atomics anywhere: the same inputs give the same bits.
// Workspace: tiles * (C Cin taps + C) floats (msmc_side_front_bwd_workspace).
//
// ---- msmc_pool_add_fwd / _bwd (pa_fwd_kernel, pa_bwd_kernel) -------------------------------------------------------------------
// pooled[b][u][c] = (((side[b][u s][c] + side[b][u s + 1][c]) + ...) over the n = min(s, Tin - u s) frames of window u, in
// ascending frame) / (float)n -- F.avg_pool1d(kernel = stride = s, ceil_mode = True, padding = 0): the last window divides by
// the frames it has.  out[b][u][c] = feat + cast(pooled): for bf16 feat the pooled value is rounded to bf16 first and the sum
// (exact in fp32 up to its one rounding) rounded again -- the bits of ``feat + pooled.to(feat.dtype)``.  s == 1: out = feat +
// cast(side), nothing is pooled and ``pooled`` is not touched.  Backward: gside[b][t][c] = fl(fl(gout[b][t / s][c] +
// gpooled[b][t / s][c]) / (float)n) -- either gradient may be absent (NULL), then it is the other alone; every element of
// gside is written exactly once, windows do not overlap.  The gradient of feat is gout itself (no launch).
// Both are streaming kernels: 4 channels per work-item as one 16-byte (fp32) / 8-byte (bf16) access where C % 4 == 0 and the
// operands are aligned for it, one channel otherwise; grid = pieces / 256, at most 8 workgroups per CU, then a stride.
#include <msmc_rt.hpp>
#include <msmc_hip.h>

#include "elem.inc"

#define SF_WG 256
#define SF_FT 32                         // frames of a tile (forward and backward)
#define SF_MAX_CIN 8
#define SF_MAX_TAPS 15
#define SF_MAX_WEIGHT 12288              // floats of weight + bias staged in LDS (48 KB)

// the input frames [t0 - pad, t0 + SF_FT + pad) of utterance b as xs[frame][ci], zeros outside [0, T)
MSMC_DEV void sf_stage_x(float* xs, const float* __restrict__ pitch, const float* __restrict__ energy, long b, int t0, int T,
                         int P, int E, int pad, int nfr) {
    const int Cin = P + E;
    for (int e = threadIdx.x; e < nfr * Cin; e += SF_WG) {
        const int f = e / Cin, ci = e - f * Cin;
        const int t = t0 - pad + f;
        float v = 0.f;
        if (t >= 0 && t < T) v = ci < P ? pitch[(b * T + t) * P + ci] : energy[(b * T + t) * E + (ci - P)];
        xs[e] = v;
    }
}

template <typename TO>
__global__ __launch_bounds__(SF_WG) void sf_fwd_kernel(const float* __restrict__ pitch, const float* __restrict__ energy,
                                                      const float* __restrict__ w, const float* __restrict__ bias,
                                                      TO* __restrict__ y, int T, int P, int E, int C, int taps, int tiles) {
    MSMC_DYN_LDS(smem);
    const int Cin = P + E, pad = (taps - 1) / 2, CT = Cin * taps;
    float* wl = (float*)smem;            // [CT][C]
    float* bl = wl + (long)CT * C;       // [C]
    float* xs = bl + C;                  // [SF_FT + taps - 1][Cin]
    const long b = (long)blockIdx.x / tiles;
    const int t0 = ((int)blockIdx.x - (int)b * tiles) * SF_FT;
    for (int e = threadIdx.x; e < CT * C; e += SF_WG) {
        const int c = e / CT, r = e - c * CT;                        // (a coalesced read of w [C][Cin][taps])
        wl[r * C + c] = w[e];
    }
    for (int c = threadIdx.x; c < C; c += SF_WG) bl[c] = bias[c];
    sf_stage_x(xs, pitch, energy, b, t0, T, P, E, pad, SF_FT + taps - 1);
    __syncthreads();
    const int CG = C / 8;
    const int nf = T - t0 < SF_FT ? T - t0 : SF_FT;
    for (int e = threadIdx.x; e < nf * CG; e += SF_WG) {
        const int f = e / CG, c0 = (e - f * CG) * 8;
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = bl[c0 + j];
        for (int ci = 0; ci < Cin; ++ci)
            for (int k = 0; k < taps; ++k) {
                const float x = xs[(f + k) * Cin + ci];
                const float* wr = wl + (ci * taps + k) * C + c0;
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] = acc[j] + wr[j] * x;
            }
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = tanhf(acc[j]);
        el_stv<8>(y, ((b * T + t0 + f) * (long)C) + c0, acc);
    }
}

template <typename TO>
__global__ __launch_bounds__(SF_WG) void sf_bwd_kernel(const float* __restrict__ pitch, const float* __restrict__ energy,
                                                      const TO* __restrict__ y, const TO* __restrict__ gy, float* __restrict__ part,
                                                      int T, int P, int E, int C, int taps, int tiles) {
    MSMC_DYN_LDS(smem);
    const int Cin = P + E, pad = (taps - 1) / 2, CT = Cin * taps;
    float* xs = (float*)smem;            // [SF_FT + taps - 1][Cin]
    const long b = (long)blockIdx.x / tiles;
    const int t0 = ((int)blockIdx.x - (int)b * tiles) * SF_FT;
    sf_stage_x(xs, pitch, energy, b, t0, T, P, E, pad, SF_FT + taps - 1);
    __syncthreads();
    const int nf = T - t0 < SF_FT ? T - t0 : SF_FT;
    float* mine = part + (long)blockIdx.x * ((long)C * CT + C);
    for (int item = threadIdx.x; item < Cin * C; item += SF_WG) {
        const int ci = item / C, c = item - ci * C;
        float s[SF_MAX_TAPS];
#pragma unroll
        for (int k = 0; k < SF_MAX_TAPS; ++k) s[k] = 0.f;
        float sb = 0.f;
        for (int f = 0; f < nf; ++f) {
            const long at = (b * T + t0 + f) * (long)C + c;
            const float yv = el_ld(y, at), g = el_ld(gy, at);
            const float dz = g * (1.f - yv * yv);
            sb = sb + dz;
#pragma unroll
            for (int k = 0; k < SF_MAX_TAPS; ++k)
                if (k < taps) s[k] = s[k] + dz * xs[(f + k) * Cin + ci];
        }
#pragma unroll
        for (int k = 0; k < SF_MAX_TAPS; ++k)
            if (k < taps) mine[(long)c * CT + ci * taps + k] = s[k];
        if (ci == 0) mine[(long)C * CT + c] = sb;
    }
}

// element e of (dw | db): the tiles' partials in ascending tile index
__global__ __launch_bounds__(SF_WG) void sf_bwd_sum_kernel(const float* __restrict__ part, float* __restrict__ dw, float* __restrict__ db,
                                                          long ntiles, int ndw, int C) {
    const int per = ndw + C;
    for (int e = blockIdx.x * SF_WG + threadIdx.x; e < per; e += gridDim.x * SF_WG) {
        float s = 0.f;
        for (long t = 0; t < ntiles; ++t) s = s + part[t * per + e];
        if (e < ndw) dw[e] = s;
        else db[e - ndw] = s;
    }
}

// one work-item per V channels of an output row; total = B * Tout * (C / V)
template <typename TF, int V>
__global__ __launch_bounds__(256) void pa_fwd_kernel(const float* __restrict__ side, const TF* __restrict__ feat,
                                                    float* __restrict__ pooled, TF* __restrict__ out, int Tin, int Tout, int C,
                                                    int scale, long total) {
    const int CV = C / V;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long row = e / CV;                                     // b Tout + u
        const int cv = (int)(e - row * CV);
        const long b = row / Tout;
        const int u = (int)(row - b * Tout);
        const int f0 = u * scale;
        const int n = Tin - f0 < scale ? Tin - f0 : scale;
        const float* src = side + ((b * Tin + f0) * (long)C) + (long)cv * V;
        float p[V], x[V];
        el_ldv<V>(src, 0L, p);
        for (int i = 1; i < n; ++i) {
            el_ldv<V>(src, (long)i * C, x);
#pragma unroll
            for (int j = 0; j < V; ++j) p[j] = p[j] + x[j];
        }
        if (scale > 1) {
            const float cnt = (float)n;
#pragma unroll
            for (int j = 0; j < V; ++j) p[j] = p[j] / cnt;
            el_stv<V>(pooled, e * V, p);
        }
        float fv[V];
        el_ldv<V>(feat, e * V, fv);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            float add = p[j];
            if (sizeof(TF) == 2) add = bf16_bits_to_f32(f32_to_bf16_bits(add));
            fv[j] = fv[j] + add;
        }
        el_stv<V>(out, e * V, fv);
    }
}

// one work-item per V channels of a row of gside; total = B * Tin * (C / V).  gout and gpooled: either may be NULL, not both
template <typename TG, int V>
__global__ __launch_bounds__(256) void pa_bwd_kernel(const TG* __restrict__ gout, const float* __restrict__ gpooled,
                                                    float* __restrict__ gside, int Tin, int Tout, int C, int scale, long total) {
    const int CV = C / V;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long row = e / CV;                                     // b Tin + t
        const int cv = (int)(e - row * CV);
        const long b = row / Tin;
        const int t = (int)(row - b * Tin);
        const int u = t / scale;
        const int f0 = u * scale;
        const int n = Tin - f0 < scale ? Tin - f0 : scale;
        const long at = ((b * Tout + u) * (long)C) + (long)cv * V;
        float g[V];
        if (gout) el_ldv<V>(gout, at, g);
        if (gpooled) {
            float q[V];
            el_ldv<V>(gpooled, at, q);
#pragma unroll
            for (int j = 0; j < V; ++j) g[j] = gout ? g[j] + q[j] : q[j];
        }
        if (scale > 1) {
            const float cnt = (float)n;
#pragma unroll
            for (int j = 0; j < V; ++j) g[j] = g[j] / cnt;
        }
        el_stv<V>(gside, e * V, g);
    }
}

struct sf_plan {
    int Cin, tiles;                  // input channels, tiles of an utterance
    long grid;                       // B * tiles
    size_t lds_fwd, lds_bwd, part;   // LDS bytes of the two kernels, floats of one tile's partials
};

// false for the shapes no kernel here takes
static bool sf_make_plan(int B, int T, int P, int E, int C, int taps, sf_plan& pl) {
    if (B < 1 || T < 1 || P < 0 || E < 0 || C < 8 || C % 8 != 0 || taps < 1 || taps > SF_MAX_TAPS || taps % 2 == 0) return false;
    pl.Cin = P + E;
    if (pl.Cin < 1 || pl.Cin > SF_MAX_CIN) return false;
    const long nw = (long)C * pl.Cin * taps + C;
    if (nw > SF_MAX_WEIGHT) return false;
    pl.tiles = (T + SF_FT - 1) / SF_FT;
    pl.grid = (long)B * pl.tiles;
    if (pl.grid > 0x7fffffffL || (long)B * T > 0x7fffffffL / C) return false;
    pl.lds_bwd = (size_t)(SF_FT + taps - 1) * pl.Cin * sizeof(float);
    pl.lds_fwd = (size_t)nw * sizeof(float) + pl.lds_bwd;
    pl.part = (size_t)nw;
    return true;
}

// 4 channels per access: the operands of the run-time dtype aligned for four elements, the fp32 ones to 16 bytes
static inline int pa_vec(size_t typed, int dtype, size_t f32s, int C) {
    return (C % 4 == 0 && msmc_aligned4(typed, dtype) && (f32s & 15) == 0) ? 4 : 1;
}
static inline bool pa_shape(int B, int Tin, int Tout, int C, int scale) {
    return B >= 1 && Tin >= 1 && C >= 1 && scale >= 1 && Tout == (Tin + scale - 1) / scale && (long)B * Tin <= 0x7fffffffL / C;
}
static inline long pa_grid(long total) {
    long blocks = (total + 255) / 256;
    return blocks > 8L * MSMC_NUM_CU ? 8L * MSMC_NUM_CU : blocks;
}

#define PA_BY_PATH(dtype, V, GO)                        \
    do {                                                \
        if ((dtype) == 0) {                             \
            if ((V) == 4) GO(float, 4);                 \
            else GO(float, 1);                          \
        } else {                                        \
            if ((V) == 4) GO(unsigned short, 4);        \
            else GO(unsigned short, 1);                 \
        }                                               \
    } while (0)

extern "C" {

size_t msmc_side_front_bwd_workspace(int B, int T, int P, int E, int C, int taps) {
    sf_plan pl;
    return sf_make_plan(B, T, P, E, C, taps, pl) ? (size_t)pl.grid * pl.part * sizeof(float) : 0;
}

int msmc_side_front_fwd(const float* pitch, const float* energy, const float* w, const float* bias, void* y, int y_dtype, int B, int T,
                        int P, int E, int C, int taps, msmc_stream stream) {
    sf_plan pl;
    if (!sf_make_plan(B, T, P, E, C, taps, pl) || !w || !bias || !y || (P > 0 && !pitch) || (E > 0 && !energy) ||
        ((uintptr_t)y & 15) != 0)
        return MSMC_E_SHAPE;
#define SF_GO(T_)                                                                                                               \
    MSMC_LAUNCH(sf_fwd_kernel<T_>, dim3((unsigned)pl.grid), dim3(SF_WG), pl.lds_fwd, (msmc_stream_t)stream, pitch, energy, w, bias, \
                (T_*)y, T, P, E, C, taps, pl.tiles)
    MSMC_BY_DTYPE(y_dtype, SF_GO);
#undef SF_GO
    return msmc_check_launch();
}

int msmc_side_front_bwd(const float* pitch, const float* energy, const void* y, const void* gy, int y_dtype, float* dw, float* db,
                        void* workspace, size_t workspace_bytes, int B, int T, int P, int E, int C, int taps, msmc_stream stream) {
    sf_plan pl;
    if (!sf_make_plan(B, T, P, E, C, taps, pl) || !y || !gy || !dw || !db || (P > 0 && !pitch) || (E > 0 && !energy) ||
        (y_dtype != 0 && y_dtype != 1))
        return MSMC_E_SHAPE;
    if (!workspace || ((uintptr_t)workspace & 15) != 0 || workspace_bytes < (size_t)pl.grid * pl.part * sizeof(float))
        return MSMC_E_WORKSPACE;
    msmc_stream_t st = (msmc_stream_t)stream;
    float* part = (float*)workspace;
#define SF_GO(T_)                                                                                                             \
    MSMC_LAUNCH(sf_bwd_kernel<T_>, dim3((unsigned)pl.grid), dim3(SF_WG), pl.lds_bwd, st, pitch, energy, (const T_*)y, (const T_*)gy, \
                part, T, P, E, C, taps, pl.tiles)
    MSMC_BY_DTYPE(y_dtype, SF_GO);
#undef SF_GO
    const int rc = msmc_check_launch();
    if (rc) return rc;
    const int ndw = C * pl.Cin * taps;
    MSMC_LAUNCH(sf_bwd_sum_kernel, dim3((unsigned)((ndw + C + SF_WG - 1) / SF_WG)), dim3(SF_WG), 0, st, (const float*)part, dw, db,
                pl.grid, ndw, C);
    return msmc_check_launch();
}

int msmc_pool_add_fwd(const float* side, const void* feat, int feat_dtype, float* pooled, void* out, int B, int Tin, int Tout, int C,
                      int scale, msmc_stream stream) {
    if (!pa_shape(B, Tin, Tout, C, scale) || !side || !feat || !out || (scale > 1 && !pooled) || (feat_dtype != 0 && feat_dtype != 1))
        return MSMC_E_SHAPE;
    const int V = pa_vec((uintptr_t)feat | (uintptr_t)out, feat_dtype, (uintptr_t)side | (uintptr_t)pooled, C);
    const long total = (long)B * Tout * (C / V);
#define PA_GO(T_, V_)                                                                                                       \
    MSMC_LAUNCH((pa_fwd_kernel<T_, V_>), dim3((unsigned)pa_grid(total)), dim3(256), 0, (msmc_stream_t)stream, side, (const T_*)feat, \
                pooled, (T_*)out, Tin, Tout, C, scale, total)
    PA_BY_PATH(feat_dtype, V, PA_GO);
#undef PA_GO
    return msmc_check_launch();
}

int msmc_pool_add_bwd(const void* gout, int gout_dtype, const float* gpooled, float* gside, int B, int Tin, int Tout, int C, int scale,
                      msmc_stream stream) {
    if (!pa_shape(B, Tin, Tout, C, scale) || (!gout && !gpooled) || !gside || (gout_dtype != 0 && gout_dtype != 1)) return MSMC_E_SHAPE;
    const int V = pa_vec((uintptr_t)gout, gout_dtype, (uintptr_t)gside | (uintptr_t)gpooled, C);
    const long total = (long)B * Tin * (C / V);
#define PA_GO(T_, V_)                                                                                                         \
    MSMC_LAUNCH((pa_bwd_kernel<T_, V_>), dim3((unsigned)pa_grid(total)), dim3(256), 0, (msmc_stream_t)stream, (const T_*)gout, gpooled, \
                gside, Tin, Tout, C, scale, total)
    PA_BY_PATH(gout_dtype, V, PA_GO);
#undef PA_GO
    return msmc_check_launch();
}

}  // extern "C"
