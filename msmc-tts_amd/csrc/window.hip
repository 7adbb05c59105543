// window.hip -- fixed-length windows of a subset of utterances, and the adjoint, for gfx950.
//
// EmbVQGANTrainer (reference msmctts/trainers/emb_vqgan_trainer.py:41-56) picks n <= B utterances of the batch and cuts one window
// of W rows from each: out[j][t][c] = x[u_j][s_j + t][c], with (u_j, s_j) read from a device table.  The forward kernel writes
// the windows in the consumer's dtype (one rounding, the bits of torch.Tensor.to) and layout ([n][W][C] IS the channels-last
// [n, 1, W, C] image the vocoder's first convolution reads); the backward kernel writes EVERY element of gx [B][T][C] once --
// the gradient row of the window that covers it, or zero -- with plain stores: no zero-fill launch, no atomics.  Both are pure
// copies (no reuse, nothing staged): 8 channels per work-item as 16-byte accesses when C % 8 == 0, one channel otherwise.
//
// The table lives on the device, so nothing here trusts it: an utterance outside [0, B) or a row outside [0, T) is never read
// (forward: zeros; backward: that window covers nothing), and every address is formed from indices checked against the
// buffer's own shape.  The backward kernel relies on each utterance being named at most once (the caller's contract: strictly
// increasing utterance indices); with duplicates the LAST entry naming an utterance wins, still within bounds.
#include <msmc_rt.hpp>
#include <msmc_hip.h>
#include "elem.inc"

// V consecutive elements (V = 8: 16-byte aligned) from src[si..] in its dtype to dst[di..] in its dtype; !valid: zeros
template <int SBF, int DBF, int V>
MSMC_DEV void wg_copy(const void* __restrict__ src, long si, void* __restrict__ dst, long di, bool valid) {
    if (V == 1) {
        if (SBF == DBF) {
            if (SBF) ((unsigned short*)dst)[di] = valid ? ((const unsigned short*)src)[si] : (unsigned short)0;
            else ((unsigned int*)dst)[di] = valid ? ((const unsigned int*)src)[si] : 0u;
        } else if (SBF) {
            el_st((float*)dst + di, valid ? el_ld((const unsigned short*)src + si) : 0.f);
        } else {
            el_st((unsigned short*)dst + di, valid ? el_ld((const float*)src + si) : 0.f);
        }
        return;
    }
    const u32x4 zero = {0u, 0u, 0u, 0u};
    if (SBF && DBF) {
        *(u32x4*)((unsigned short*)dst + di) = valid ? *(const u32x4*)((const unsigned short*)src + si) : zero;
    } else if (!SBF && !DBF) {
        const u32x4* s = (const u32x4*)((const float*)src + si);
        u32x4* d = (u32x4*)((float*)dst + di);
        const u32x4 a = valid ? s[0] : zero, b = valid ? s[1] : zero;
        d[0] = a;
        d[1] = b;
    } else if (SBF) {                                     // bf16 -> fp32: exact
        const u32x4 r = valid ? *(const u32x4*)((const unsigned short*)src + si) : zero;
        u32x4 lo, hi;
        lo[0] = r[0] << 16; lo[1] = r[0] & 0xffff0000u; lo[2] = r[1] << 16; lo[3] = r[1] & 0xffff0000u;
        hi[0] = r[2] << 16; hi[1] = r[2] & 0xffff0000u; hi[2] = r[3] << 16; hi[3] = r[3] & 0xffff0000u;
        u32x4* d = (u32x4*)((float*)dst + di);
        d[0] = lo;
        d[1] = hi;
    } else {                                              // fp32 -> bf16: round to nearest even
        const f32x4* s = (const f32x4*)((const float*)src + si);
        const f32x4 fz = {0.f, 0.f, 0.f, 0.f};
        const f32x4 a = valid ? s[0] : fz, b = valid ? s[1] : fz;
        u32x4 r;
        r[0] = pack_bf16x2(a[0], a[1]);
        r[1] = pack_bf16x2(a[2], a[3]);
        r[2] = pack_bf16x2(b[0], b[1]);
        r[3] = pack_bf16x2(b[2], b[3]);
        *(u32x4*)((unsigned short*)dst + di) = r;
    }
}

// one work-item per V channels of an output row; total = n * W * (C / V)
template <int XBF, int OBF, int V>
__global__ __launch_bounds__(256) void window_gather_fwd_kernel(const void* __restrict__ x, const int* __restrict__ win,
                                                               void* __restrict__ out, int B, int T, int C, int W, long total) {
    const int CV = C / V;
    const long per = (long)W * CV;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long j = e / per, r = e - j * per;
        const int t = (int)(r / CV), cv = (int)(r - (long)t * CV);
        const int u = win[2 * j];
        const long row = (long)win[2 * j + 1] + t;
        const bool valid = u >= 0 && u < B && row >= 0 && row < T;
        wg_copy<XBF, OBF, V>(x, valid ? ((long)u * T + row) * C + (long)cv * V : 0, out, e * V, valid);
    }
}

// blockIdx.x = utterance * bpu + chunk: the workgroups of an utterance stride over its T * (C / V) pieces, every piece written
template <int GBF, int XBF, int V>
__global__ __launch_bounds__(256) void window_gather_bwd_kernel(const void* __restrict__ gout, const int* __restrict__ win,
                                                               void* __restrict__ gx, int T, int C, int n, int W, int bpu) {
    const int b = (int)blockIdx.x / bpu, chunk = (int)blockIdx.x - b * bpu;
    int j = -1;
    long s = 0;
    for (int k = 0; k < n; ++k)                           // (n <= B entries, the same walk in every lane)
        if (win[2 * k] == b) {
            j = k;
            s = win[2 * k + 1];
        }
    const int CV = C / V;
    const long per = (long)T * CV;
    for (long e = (long)chunk * 256 + threadIdx.x; e < per; e += (long)bpu * 256) {
        const int t = (int)(e / CV), cv = (int)(e - (long)t * CV);
        const long r = (long)t - s;
        const bool valid = j >= 0 && r >= 0 && r < W;
        wg_copy<GBF, XBF, V>(gout, valid ? ((long)j * W + r) * C + (long)cv * V : 0, gx, ((long)b * per + e) * V, valid);
    }
}

static inline bool wg_bad_shape(const void* a, const int* win, const void* b, int fa, int fb, int B, int T, int C, int n, int W) {
    return !a || !win || !b || (fa | fb) < 0 || fa > 1 || fb > 1 || B < 1 || T < 1 || C < 1 || n < 1 || n > B || W < 1;
}
static inline int wg_vec(const void* a, const void* b, int C) {
    return (C % 8 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0) ? 8 : 1;
}

#define WG_DISPATCH(LAUNCH)                          \
    do {                                             \
        if (V == 8) {                                \
            if (!sbf && !dbf) LAUNCH(0, 0, 8);       \
            else if (!sbf) LAUNCH(0, 1, 8);          \
            else if (!dbf) LAUNCH(1, 0, 8);          \
            else LAUNCH(1, 1, 8);                    \
        } else {                                     \
            if (!sbf && !dbf) LAUNCH(0, 0, 1);       \
            else if (!sbf) LAUNCH(0, 1, 1);          \
            else if (!dbf) LAUNCH(1, 0, 1);          \
            else LAUNCH(1, 1, 1);                    \
        }                                            \
    } while (0)

extern "C" {

int msmc_window_gather_fwd(const void* x, int x_bf16, const int* win, void* out, int out_bf16, int B, int T, int C, int n, int W,
                           msmc_stream stream) {
    if (wg_bad_shape(x, win, out, x_bf16, out_bf16, B, T, C, n, W)) return MSMC_E_SHAPE;
    const int V = wg_vec(x, out, C), sbf = x_bf16, dbf = out_bf16;
    const long total = (long)n * W * (C / V);
    long blocks = (total + 255) / 256;
    if (blocks > 8L * MSMC_NUM_CU) blocks = 8L * MSMC_NUM_CU;
#define WG_FWD(S, D, VV) \
    MSMC_LAUNCH((window_gather_fwd_kernel<S, D, VV>), dim3((unsigned)blocks), dim3(256), 0, (msmc_stream_t)stream, x, win, out, B, T, C, W, total)
    WG_DISPATCH(WG_FWD);
#undef WG_FWD
    return msmc_check_launch();
}

int msmc_window_gather_bwd(const void* gout, int gout_bf16, const int* win, void* gx, int gx_bf16, int B, int T, int C, int n, int W,
                           msmc_stream stream) {
    if (wg_bad_shape(gout, win, gx, gout_bf16, gx_bf16, B, T, C, n, W)) return MSMC_E_SHAPE;
    const int V = wg_vec(gout, gx, C), sbf = gout_bf16, dbf = gx_bf16;
    const long per = (long)T * (C / V);
    long bpu = (per + 255) / 256, cap = 8L * MSMC_NUM_CU / B;            // workgroups per utterance
    if (cap < 1) cap = 1;
    if (bpu > cap) bpu = cap;
    if ((long)B * bpu > 0x7fffffffL) return MSMC_E_SHAPE;
#define WG_BWD(S, D, VV)                                                                                                            \
    MSMC_LAUNCH((window_gather_bwd_kernel<S, D, VV>), dim3((unsigned)(B * bpu)), dim3(256), 0, (msmc_stream_t)stream, gout, win, gx, T, C, \
                n, W, (int)bpu)
    WG_DISPATCH(WG_BWD);
#undef WG_BWD
    return msmc_check_launch();
}

}  // extern "C"
