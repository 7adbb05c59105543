// tdnn.hip -- the operators of the speaker reference encoder (ECAPA-TDNN, reference msmctts/networks/vqgantts/tdnn.py:67-244)
// that are passes over channels-last frames x [B][T][C]:
//   ReLU + affine BatchNorm       y = gamma (relu(x) - mean) rstd + beta                            tdnn.py:96-98, 115-116
//   squeeze-excitation + residual y = res + x sigmoid(W2 relu(W1 mean_t(x) + b1) + b2)              tdnn.py:122-134, 150-151
//   attentive statistics pooling  (sum_t alpha x | sqrt(max(sum_t alpha x^2 - mean^2, 1e-9))), alpha = softmax_t(a)   tdnn.py:163-170
// Activations fp32 (dtype 0) or bf16 (dtype 1); every statistic, sum and parameter gradient in fp32.  A row is read as 16-byte
// vectors (V = 4 fp32 / 8 bf16 channels per lane).  A workgroup owns a slab of rows of one chunk of at most 64 lanes' worth of
// channels (grid y) and keeps R = min(256 / lanes, 32) rows in flight.  Every reduction runs in a fixed order -- a lane walks
// its rows in order, the R lanes of a channel are merged in order through LDS, the slabs are merged in order from a workspace --
// and there are no atomics: two calls on the same input are bit-identical, and the passes can be captured.
#include <msmc_rt.hpp>
#include <msmc_hip.h>
#include "bn_common.inc"

// lane geometry of a workgroup: GL lanes per row of this chunk, R rows in flight, this lane = (rr, cg) and its first channel c0
struct td_lanes { int GL, R, rr, cg, c0; bool live; };
template <int V> MSMC_DEV td_lanes td_geometry(int C) {
    td_lanes l;
    const int G = C / V;
    l.GL = G < 64 ? G : 64;
    l.R = 256 / l.GL < 32 ? 256 / l.GL : 32;
    l.rr = (int)threadIdx.x / l.GL;
    l.cg = (int)threadIdx.x - l.rr * l.GL;
    const int gcg = (int)blockIdx.y * l.GL + l.cg;
    l.c0 = gcg * V;
    l.live = l.rr < l.R && gcg < G;
    return l;
}
static int td_chunks(int C, int V) {
    const int G = C / V, GL = G < 64 ? G : 64;
    return (G + GL - 1) / GL;
}
static int td_vec(int dtype) { return dtype == 0 ? 4 : 8; }
#define TD_LDS(l, q) (((l).rr * (l).GL + (l).cg) * V + (q))
#define TD_LDS_ROW(l, j, q) (((j) * (l).GL + (l).cg) * V + (q))

// ---- ReLU + affine BatchNorm ----------------------------------------------------------------------------------------------
// rows x [N][C] at a row stride of ldx elements (a channel slice of a wider row).  Welford / Chan as msmc_bn_*, on relu(x).
// launch (a): ws[b][0][c] = mean, ws[b][1][c] = M2 of relu(x) over slab b, counts[b] behind the nblk x 2 x C floats
template <typename T>
__global__ __launch_bounds__(256) void rbn_stats_kernel(const T* __restrict__ x, long ldx, float* __restrict__ ws, long N, int C,
                                                        long slab, int nblk) {
    constexpr int V = bn_vec<T>::V;
    __shared__ float s_mean[256 * V], s_m2[256 * V];
    __shared__ float s_n[32];
    const td_lanes l = td_geometry<V>(C);
    const long r0 = (long)blockIdx.x * slab, r1 = r0 + slab < N ? r0 + slab : N;
    float mean[V], m2[V];
#pragma unroll
    for (int q = 0; q < V; ++q) mean[q] = m2[q] = 0.f;
    int n = 0;
    if (l.live) {
#pragma unroll 4
        for (long row = r0 + l.rr; row < r1; row += l.R) {
            float v[V];
            el_ldv(x, row * ldx + l.c0, v);
            n = n + 1;
            const float inv = 1.f / (float)n;
#pragma unroll
            for (int q = 0; q < V; ++q) {
                const float r = v[q] > 0.f ? v[q] : 0.f;
                const float d = r - mean[q];
                mean[q] = mean[q] + d * inv;
                m2[q] = m2[q] + d * (r - mean[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < V; ++q) {
            s_mean[TD_LDS(l, q)] = mean[q];
            s_m2[TD_LDS(l, q)] = m2[q];
        }
        if (l.cg == 0) s_n[l.rr] = (float)n;
    }
    __syncthreads();
    if (l.live && l.rr == 0) {
        float cnt[V];
#pragma unroll
        for (int q = 0; q < V; ++q) cnt[q] = (float)n;
        for (int j = 1; j < l.R; ++j) {
            const float nb = s_n[j];
#pragma unroll
            for (int q = 0; q < V; ++q) bn_chan(cnt[q], mean[q], m2[q], nb, s_mean[TD_LDS_ROW(l, j, q)], s_m2[TD_LDS_ROW(l, j, q)]);
        }
        el_stv<V>(ws, ((long)blockIdx.x * 2 + 0) * C + l.c0, mean);
        el_stv<V>(ws, ((long)blockIdx.x * 2 + 1) * C + l.c0, m2);
        if (threadIdx.x == 0 && blockIdx.y == 0) ((int*)(ws + (long)nblk * 2 * C))[blockIdx.x] = (int)(r1 - r0);
    }
}

// launch (b) (ws != NULL): every workgroup merges the nblk partials in the same order, then writes its slab of y; slab 0 also
// keeps mean / rstd and advances the running statistics (unbiased variance) and the step counter.
// Evaluation (ws == NULL): the running statistics; rstd_out keeps 1 / sqrt(running_var + eps).
template <typename T>
__global__ __launch_bounds__(256) void rbn_norm_kernel(const T* __restrict__ x, long ldx, const float* __restrict__ ws, int nblk,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       T* __restrict__ y, long ldy, float* __restrict__ mean_out,
                                                       float* __restrict__ rstd_out, float* running_mean, float* running_var,
                                                       long long* num_batches_tracked, long N, int C, long slab, float eps,
                                                       float momentum) {
    constexpr int V = bn_vec<T>::V;
    __shared__ float s_mean[256 * V], s_m2[256 * V];
    __shared__ float s_n[32];
    const td_lanes l = td_geometry<V>(C);
    float mean[V], rstd[V];
    if (ws) {
        float cnt[V], m2[V];
#pragma unroll
        for (int q = 0; q < V; ++q) cnt[q] = mean[q] = m2[q] = 0.f;
        if (l.live) {
            const int* counts = (const int*)(ws + (long)nblk * 2 * C);
            for (int j = l.rr; j < nblk; j += l.R) {
                float mb[V], m2b[V];
                el_ldv<V>(ws, ((long)j * 2 + 0) * C + l.c0, mb);
                el_ldv<V>(ws, ((long)j * 2 + 1) * C + l.c0, m2b);
                const float nb = (float)counts[j];
#pragma unroll
                for (int q = 0; q < V; ++q) bn_chan(cnt[q], mean[q], m2[q], nb, mb[q], m2b[q]);
            }
#pragma unroll
            for (int q = 0; q < V; ++q) {
                s_mean[TD_LDS(l, q)] = mean[q];
                s_m2[TD_LDS(l, q)] = m2[q];
            }
            if (l.cg == 0) s_n[l.rr] = cnt[0];
        }
        __syncthreads();
        if (!l.live) return;
#pragma unroll
        for (int q = 0; q < V; ++q) cnt[q] = mean[q] = m2[q] = 0.f;
        for (int j = 0; j < l.R; ++j) {
            const float nb = s_n[j];
#pragma unroll
            for (int q = 0; q < V; ++q) bn_chan(cnt[q], mean[q], m2[q], nb, s_mean[TD_LDS_ROW(l, j, q)], s_m2[TD_LDS_ROW(l, j, q)]);
        }
#pragma unroll
        for (int q = 0; q < V; ++q) rstd[q] = 1.f / sqrtf(m2[q] / (float)N + eps);
        if (blockIdx.x == 0 && l.rr == 0) {
#pragma unroll
            for (int q = 0; q < V; ++q) {
                const int c = l.c0 + q;
                mean_out[c] = mean[q];
                rstd_out[c] = rstd[q];
                if (running_mean) {
                    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean[q];
                    running_var[c] = (1.f - momentum) * running_var[c] + momentum * (m2[q] / (float)(N - 1));
                }
            }
            if (threadIdx.x == 0 && blockIdx.y == 0 && num_batches_tracked) num_batches_tracked[0] = num_batches_tracked[0] + 1;
        }
    } else {
        if (!l.live) return;
#pragma unroll
        for (int q = 0; q < V; ++q) {
            const int c = l.c0 + q;
            mean[q] = running_mean[c];
            rstd[q] = 1.f / sqrtf(running_var[c] + eps);
            if (rstd_out && blockIdx.x == 0 && l.rr == 0) rstd_out[c] = rstd[q];
        }
    }
    float ga[V], be[V];
    el_ldv<V>(gamma, l.c0, ga);
    el_ldv<V>(beta, l.c0, be);
    const long r0 = (long)blockIdx.x * slab, r1 = r0 + slab < N ? r0 + slab : N;
#pragma unroll 4
    for (long row = r0 + l.rr; row < r1; row += l.R) {
        float v[V];
        el_ldv(x, row * ldx + l.c0, v);
#pragma unroll
        for (int q = 0; q < V; ++q) v[q] = (((v[q] > 0.f ? v[q] : 0.f) - mean[q]) * rstd[q]) * ga[q] + be[q];
        el_stv(y, row * ldy + l.c0, v);
    }
}

// backward, launch one: ws[b][0][c] = sum g, ws[b][1][c] = sum g xhat over slab b, xhat = (relu(x) - mean) rstd recomputed
template <typename T>
__global__ __launch_bounds__(256) void rbn_bwd_stats_kernel(const T* __restrict__ g, long ldg, const T* __restrict__ x, long ldx,
                                                            const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
                                                            float* __restrict__ ws, long N, int C, long slab) {
    constexpr int V = bn_vec<T>::V;
    __shared__ float s_1[256 * V], s_2[256 * V];
    const td_lanes l = td_geometry<V>(C);
    const long r0 = (long)blockIdx.x * slab, r1 = r0 + slab < N ? r0 + slab : N;
    float s1[V], s2[V];
#pragma unroll
    for (int q = 0; q < V; ++q) s1[q] = s2[q] = 0.f;
    if (l.live) {
        float mean[V], rstd[V];
        el_ldv<V>(mean_in, l.c0, mean);
        el_ldv<V>(rstd_in, l.c0, rstd);
#pragma unroll 4
        for (long row = r0 + l.rr; row < r1; row += l.R) {
            float v[V], gv[V];
            el_ldv(x, row * ldx + l.c0, v);
            el_ldv(g, row * ldg + l.c0, gv);
#pragma unroll
            for (int q = 0; q < V; ++q) {
                s1[q] = s1[q] + gv[q];
                s2[q] = s2[q] + gv[q] * (((v[q] > 0.f ? v[q] : 0.f) - mean[q]) * rstd[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < V; ++q) {
            s_1[TD_LDS(l, q)] = s1[q];
            s_2[TD_LDS(l, q)] = s2[q];
        }
    }
    __syncthreads();
    if (l.live && l.rr == 0) {
        for (int j = 1; j < l.R; ++j)
#pragma unroll
            for (int q = 0; q < V; ++q) {
                s1[q] = s1[q] + s_1[TD_LDS_ROW(l, j, q)];
                s2[q] = s2[q] + s_2[TD_LDS_ROW(l, j, q)];
            }
        el_stv<V>(ws, ((long)blockIdx.x * 2 + 0) * C + l.c0, s1);
        el_stv<V>(ws, ((long)blockIdx.x * 2 + 1) * C + l.c0, s2);
    }
}

// backward, launch two (ws != NULL): the partials added in the same order by every workgroup; slab 0 writes dbeta = sum g and
// dgamma = sum g xhat; training: gx = [x > 0] gamma rstd (g - sum g / N - xhat sum(g xhat) / N); EVAL: gx = [x > 0] gamma rstd g
// (ws == NULL: no parameter gradients, one launch)
template <typename T, bool EVAL>
__global__ __launch_bounds__(256) void rbn_bwd_apply_kernel(const T* __restrict__ g, long ldg, const T* __restrict__ x, long ldx,
                                                            const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
                                                            const float* __restrict__ gamma, const float* __restrict__ ws, int nblk,
                                                            T* __restrict__ gx, long ldgx, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta, long N, int C, long slab) {
    constexpr int V = bn_vec<T>::V;
    __shared__ float s_1[256 * V], s_2[256 * V];
    const td_lanes l = td_geometry<V>(C);
    float s1[V], s2[V];
#pragma unroll
    for (int q = 0; q < V; ++q) s1[q] = s2[q] = 0.f;
    if (ws) {
        if (l.live) {
            for (int j = l.rr; j < nblk; j += l.R) {
                float a[V], b[V];
                el_ldv<V>(ws, ((long)j * 2 + 0) * C + l.c0, a);
                el_ldv<V>(ws, ((long)j * 2 + 1) * C + l.c0, b);
#pragma unroll
                for (int q = 0; q < V; ++q) { s1[q] = s1[q] + a[q]; s2[q] = s2[q] + b[q]; }
            }
#pragma unroll
            for (int q = 0; q < V; ++q) {
                s_1[TD_LDS(l, q)] = s1[q];
                s_2[TD_LDS(l, q)] = s2[q];
            }
        }
        __syncthreads();
        if (!l.live) return;
#pragma unroll
        for (int q = 0; q < V; ++q) s1[q] = s2[q] = 0.f;
        for (int j = 0; j < l.R; ++j)
#pragma unroll
            for (int q = 0; q < V; ++q) {
                s1[q] = s1[q] + s_1[TD_LDS_ROW(l, j, q)];
                s2[q] = s2[q] + s_2[TD_LDS_ROW(l, j, q)];
            }
        if (blockIdx.x == 0 && l.rr == 0 && dgamma) {
            el_stv<V>(dbeta, l.c0, s1);
            el_stv<V>(dgamma, l.c0, s2);
        }
    } else if (!l.live) {
        return;
    }
    float mean[V], rstd[V], ga[V];
    el_ldv<V>(mean_in, l.c0, mean);
    el_ldv<V>(rstd_in, l.c0, rstd);
    el_ldv<V>(gamma, l.c0, ga);
#pragma unroll
    for (int q = 0; q < V; ++q) { s1[q] = s1[q] / (float)N; s2[q] = s2[q] / (float)N; }
    const long r0 = (long)blockIdx.x * slab, r1 = r0 + slab < N ? r0 + slab : N;
#pragma unroll 4
    for (long row = r0 + l.rr; row < r1; row += l.R) {
        float v[V], gv[V];
        el_ldv(x, row * ldx + l.c0, v);
        el_ldv(g, row * ldg + l.c0, gv);
#pragma unroll
        for (int q = 0; q < V; ++q) {
            const float r = v[q] > 0.f ? v[q] : 0.f;
            float d;
            if constexpr (EVAL) d = (ga[q] * rstd[q]) * gv[q];
            else d = (ga[q] * rstd[q]) * ((gv[q] - s1[q]) - ((r - mean[q]) * rstd[q]) * s2[q]);
            v[q] = v[q] > 0.f ? d : 0.f;
        }
        el_stv(gx, row * ldgx + l.c0, v);
    }
}

// ---- squeeze-excitation ---------------------------------------------------------------------------------------------------
// per-slab time sums of one batch element (grid: slabs x chunks x B): ws[b][slab][c] = sum_t a (MUL: sum_t a b)
template <typename T, bool MUL>
__global__ __launch_bounds__(256) void se_sums_kernel(const T* __restrict__ a, const T* __restrict__ b, float* __restrict__ ws,
                                                      int Tn, int C, int slab) {
    constexpr int V = bn_vec<T>::V;
    __shared__ float s_1[256 * V];
    const td_lanes l = td_geometry<V>(C);
    const long base = (long)blockIdx.z * Tn * C;
    const int r0 = (int)blockIdx.x * slab, r1 = r0 + slab < Tn ? r0 + slab : Tn;
    float s[V];
#pragma unroll
    for (int q = 0; q < V; ++q) s[q] = 0.f;
    if (l.live) {
#pragma unroll 4
        for (int row = r0 + l.rr; row < r1; row += l.R) {
            float v[V];
            el_ldv(a, base + (long)row * C + l.c0, v);
            if constexpr (MUL) {
                float w[V];
                el_ldv(b, base + (long)row * C + l.c0, w);
#pragma unroll
                for (int q = 0; q < V; ++q) v[q] = v[q] * w[q];
            }
#pragma unroll
            for (int q = 0; q < V; ++q) s[q] = s[q] + v[q];
        }
#pragma unroll
        for (int q = 0; q < V; ++q) s_1[TD_LDS(l, q)] = s[q];
    }
    __syncthreads();
    if (l.live && l.rr == 0) {
        for (int j = 1; j < l.R; ++j)
#pragma unroll
            for (int q = 0; q < V; ++q) s[q] = s[q] + s_1[TD_LDS_ROW(l, j, q)];
        el_stv<V>(ws, ((long)blockIdx.z * gridDim.x + blockIdx.x) * C + l.c0, s);
    }
}

// out[b][c] = sum over the slabs, in order (the gate's gradient sum_t g x)
__global__ __launch_bounds__(256) void se_merge_kernel(const float* __restrict__ ws, int nslab, float* __restrict__ out, int B, int C) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= B * C) return;
    const int b = i / C, c = i - b * C;
    float acc = 0.f;
    for (int j = 0; j < nslab; ++j) acc = acc + ws[((long)b * nslab + j) * C + c];
    out[i] = acc;
}

// one workgroup per batch element: time mean from the slab sums (in order), hidden = relu(W1 mean + b1), gate = sigmoid(W2 hidden
// + b2).  A wave owns an output row: its lanes stride over the inputs and add up with wave_sum.  mean / hidden are kept for the
// backward pass of the two small layers.
__global__ __launch_bounds__(256) void se_gate_kernel(const float* __restrict__ ws, int nslab, const float* __restrict__ W1,
                                                      const float* __restrict__ b1, const float* __restrict__ W2,
                                                      const float* __restrict__ b2, float* __restrict__ gate,
                                                      float* __restrict__ mean_out, float* __restrict__ hid_out, int Tn, int C) {
    __shared__ float s_s[1024], s_h[512];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, H = C / 2;
    for (int c = tid; c < C; c += 256) {
        float acc = 0.f;
        for (int j = 0; j < nslab; ++j) acc = acc + ws[((long)b * nslab + j) * C + c];
        acc = acc / (float)Tn;
        s_s[c] = acc;
        mean_out[(long)b * C + c] = acc;
    }
    __syncthreads();
    const int wave = tid / MSMC_WAVE, lane = tid - wave * MSMC_WAVE;
    for (int j = wave; j < H; j += 256 / MSMC_WAVE) {
        float p = 0.f;
        for (int c = lane; c < C; c += MSMC_WAVE) p = p + W1[(long)j * C + c] * s_s[c];
        p = wave_sum(p) + b1[j];
        p = p > 0.f ? p : 0.f;
        if (lane == 0) {
            s_h[j] = p;
            hid_out[(long)b * H + j] = p;
        }
    }
    __syncthreads();
    for (int c = wave; c < C; c += 256 / MSMC_WAVE) {
        float p = 0.f;
        for (int j = lane; j < H; j += MSMC_WAVE) p = p + W2[(long)c * H + j] * s_h[j];
        p = wave_sum(p) + b2[c];
        if (lane == 0) gate[(long)b * C + c] = 1.f / (1.f + expf(-p));
    }
}

// y = a * gate[b] + add: add = res[b][t][c] (forward) or, ROWVEC, ds[b][c] (backward: the time-mean path, already / T)
template <typename T, bool ROWVEC>
__global__ __launch_bounds__(256) void se_scale_kernel(const T* __restrict__ a, const float* __restrict__ gate,
                                                       const void* __restrict__ add, T* __restrict__ y, int Tn, int C, int slab) {
    constexpr int V = bn_vec<T>::V;
    const td_lanes l = td_geometry<V>(C);
    if (!l.live) return;
    const long base = (long)blockIdx.z * Tn * C;
    const int r0 = (int)blockIdx.x * slab, r1 = r0 + slab < Tn ? r0 + slab : Tn;
    float gt[V], dv[V];
    el_ldv<V>(gate, (long)blockIdx.z * C + l.c0, gt);
    if constexpr (ROWVEC) el_ldv<V>((const float*)add, (long)blockIdx.z * C + l.c0, dv);
#pragma unroll 4
    for (int row = r0 + l.rr; row < r1; row += l.R) {
        float v[V];
        el_ldv(a, base + (long)row * C + l.c0, v);
        if constexpr (!ROWVEC) el_ldv((const T*)add, base + (long)row * C + l.c0, dv);
#pragma unroll
        for (int q = 0; q < V; ++q) v[q] = v[q] * gt[q] + dv[q];
        el_stv(y, base + (long)row * C + l.c0, v);
    }
}

// ---- attentive statistics pooling -----------------------------------------------------------------------------------------
// online softmax state of a channel over a run of frames: (m, l, s1, s2) = (max a, sum e^(a-m), sum e^(a-m) x, sum e^(a-m) x^2)
MSMC_DEV void asp_merge(float& m, float& l, float& s1, float& s2, float mb, float lb, float s1b, float s2b) {
    if (lb == 0.f) return;                        // an empty run
    if (l == 0.f) { m = mb; l = lb; s1 = s1b; s2 = s2b; return; }
    const float mn = m > mb ? m : mb;
    const float fa = expf(m - mn), fb = expf(mb - mn);
    l = l * fa + lb * fb;
    s1 = s1 * fa + s1b * fb;
    s2 = s2 * fa + s2b * fb;
    m = mn;
}

// grid: splits of T x chunks x B.  x and a are read once; ws[b][split][0..3][c] = (m, l, s1, s2) of the split's frames
template <typename T>
__global__ __launch_bounds__(256) void asp_part_kernel(const T* __restrict__ x, const T* __restrict__ a, float* __restrict__ ws,
                                                       int Tn, int C, int slab) {
    constexpr int V = bn_vec<T>::V;
    __shared__ float s_m[256 * V], s_l[256 * V], s_1[256 * V], s_2[256 * V];
    const td_lanes l = td_geometry<V>(C);
    const long base = (long)blockIdx.z * Tn * C;
    const int r0 = (int)blockIdx.x * slab, r1 = r0 + slab < Tn ? r0 + slab : Tn;
    float m[V], ls[V], s1[V], s2[V];
#pragma unroll
    for (int q = 0; q < V; ++q) { m[q] = -__builtin_huge_valf(); ls[q] = s1[q] = s2[q] = 0.f; }
    if (l.live) {
#pragma unroll 2
        for (int row = r0 + l.rr; row < r1; row += l.R) {
            float xv[V], av[V];
            el_ldv(x, base + (long)row * C + l.c0, xv);
            el_ldv(a, base + (long)row * C + l.c0, av);
#pragma unroll
            for (int q = 0; q < V; ++q) {
                // one exponential per element: the larger of (running maximum, new logit) keeps weight 1
                const float d = av[q] - m[q];
                const float e = expf(d > 0.f ? -d : d);
                const float sc = d > 0.f ? e : 1.f, w = d > 0.f ? 1.f : e;
                m[q] = d > 0.f ? av[q] : m[q];
                ls[q] = ls[q] * sc + w;
                s1[q] = s1[q] * sc + w * xv[q];
                s2[q] = s2[q] * sc + w * (xv[q] * xv[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < V; ++q) {
            s_m[TD_LDS(l, q)] = m[q];
            s_l[TD_LDS(l, q)] = ls[q];
            s_1[TD_LDS(l, q)] = s1[q];
            s_2[TD_LDS(l, q)] = s2[q];
        }
    }
    __syncthreads();
    if (l.live && l.rr == 0) {
        for (int j = 1; j < l.R; ++j)
#pragma unroll
            for (int q = 0; q < V; ++q)
                asp_merge(m[q], ls[q], s1[q], s2[q], s_m[TD_LDS_ROW(l, j, q)], s_l[TD_LDS_ROW(l, j, q)], s_1[TD_LDS_ROW(l, j, q)],
                          s_2[TD_LDS_ROW(l, j, q)]);
        const long o = ((long)blockIdx.z * gridDim.x + blockIdx.x) * 4 * C + l.c0;
        el_stv<V>(ws, o, m);
        el_stv<V>(ws, o + C, ls);
        el_stv<V>(ws, o + 2L * C, s1);
        el_stv<V>(ws, o + 3L * C, s2);
    }
}

// one lane per (b, c): the splits merged in order; out[b] = (mean | std), stats[b][0..3][c] = (m, l, mean, residual) for the backward
__global__ __launch_bounds__(256) void asp_merge_kernel(const float* __restrict__ ws, int nsplit, float* __restrict__ out,
                                                        float* __restrict__ stats, int B, int C) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= B * C) return;
    const int b = i / C, c = i - b * C;
    float m = 0.f, l = 0.f, s1 = 0.f, s2 = 0.f;
    for (int j = 0; j < nsplit; ++j) {
        const float* p = ws + ((long)b * nsplit + j) * 4 * C + c;
        asp_merge(m, l, s1, s2, p[0], p[C], p[2L * C], p[3L * C]);
    }
    const float mean = s1 / l, res = s2 / l - mean * mean;
    out[(long)b * 2 * C + c] = mean;
    out[(long)b * 2 * C + C + c] = sqrtf(res > 1e-9f ? res : 1e-9f);
    float* st = stats + (long)b * 4 * C + c;
    st[0] = m;
    st[C] = l;
    st[2L * C] = mean;
    st[3L * C] = res;
}

// one pass: alpha = e^(a - m) / l from the saved statistics; with dres = gstd / (2 std) (0 where the clamp is active),
// dmean = gmean - 2 mean dres:  gx = alpha (dmean + 2 dres x),  ga = alpha (dmean x + dres x^2 - (dmean mean + dres sum alpha x^2))
template <typename T>
__global__ __launch_bounds__(256) void asp_bwd_kernel(const float* __restrict__ gout, const T* __restrict__ x, const T* __restrict__ a,
                                                      const float* __restrict__ stats, T* __restrict__ gx, T* __restrict__ ga, int Tn,
                                                      int C, int slab) {
    constexpr int V = bn_vec<T>::V;
    const td_lanes l = td_geometry<V>(C);
    if (!l.live) return;
    const long base = (long)blockIdx.z * Tn * C;
    const int r0 = (int)blockIdx.x * slab, r1 = r0 + slab < Tn ? r0 + slab : Tn;
    float m[V], il[V], k0[V], k1[V], dot[V];
    {
        float ls[V], mean[V], res[V], gm[V], gs[V];
        const long s0 = (long)blockIdx.z * 4 * C + l.c0;
        el_ldv<V>(stats, s0, m);
        el_ldv<V>(stats, s0 + C, ls);
        el_ldv<V>(stats, s0 + 2L * C, mean);
        el_ldv<V>(stats, s0 + 3L * C, res);
        el_ldv<V>(gout, (long)blockIdx.z * 2 * C + l.c0, gm);
        el_ldv<V>(gout, (long)blockIdx.z * 2 * C + C + l.c0, gs);
#pragma unroll
        for (int q = 0; q < V; ++q) {
            const float dres = res[q] < 1e-9f ? 0.f : gs[q] / (2.f * sqrtf(res[q]));
            il[q] = 1.f / ls[q];
            k1[q] = dres;
            k0[q] = gm[q] - 2.f * mean[q] * dres;
            dot[q] = k0[q] * mean[q] + dres * (res[q] + mean[q] * mean[q]);
        }
    }
#pragma unroll 2
    for (int row = r0 + l.rr; row < r1; row += l.R) {
        float xv[V], av[V];
        el_ldv(x, base + (long)row * C + l.c0, xv);
        el_ldv(a, base + (long)row * C + l.c0, av);
#pragma unroll
        for (int q = 0; q < V; ++q) {
            const float al = expf(av[q] - m[q]) * il[q];
            const float xx = xv[q];
            av[q] = al * ((k0[q] * xx + k1[q] * (xx * xx)) - dot[q]);
            xv[q] = al * (k0[q] + 2.f * k1[q] * xx);
        }
        el_stv(gx, base + (long)row * C + l.c0, xv);
        el_stv(ga, base + (long)row * C + l.c0, av);
    }
}

// ---- launch geometry ------------------------------------------------------------------------------------------------------
// slabs of T frames for ``groups`` = B x chunks independent (batch element, channel chunk) pairs: reductions take at least 64
// frames per slab and about two workgroups per CU, streaming passes 32 frames and eight
static bn_grid td_slabs(int Tn, int groups, bool streaming) {
    long cap = (streaming ? 8L : 2L) * MSMC_NUM_CU / (groups > 0 ? groups : 1);
    if (cap < 1) cap = 1;
    const int per = streaming ? 32 : 64;
    long nb = ((long)Tn + per - 1) / per;
    if (nb > cap) nb = cap;
    if (nb < 1) nb = 1;
    bn_grid gr;
    gr.slab = (Tn + nb - 1) / nb;
    gr.nblk = (int)((Tn + gr.slab - 1) / gr.slab);
    return gr;
}
// the larger slab count of the two vector widths (the chunk count, hence the cap, differs): what a workspace must hold
static int td_max_slabs(int Tn, int B, int C) {
    const bn_grid g4 = td_slabs(Tn, B * td_chunks(C, 4), false), g8 = td_slabs(Tn, B * td_chunks(C, 8), false);
    return g4.nblk > g8.nblk ? g4.nblk : g8.nblk;
}
static bool td_aligned(size_t bits) { return (bits & 15) == 0; }
static bool rbn_shape_ok(long N, int C, long ld) { return bn_shape_ok(N, C) && ld >= C && (ld % 8) == 0; }
static bool se_shape_ok(int B, int Tn, int C) {
    return B > 0 && B < 65536 && Tn > 0 && C > 0 && (C % 8) == 0 && C <= 1024 && (long)B * Tn * C < (1L << 40) && (long)B * C < (1L << 31);
}
static bool asp_shape_ok(int B, int Tn, int C) {
    return B > 0 && B < 65536 && Tn > 0 && C > 0 && (C % 8) == 0 && C <= 1536 && (long)B * Tn * C < (1L << 40) && (long)B * C < (1L << 31);
}
#define TD_P(p) ((size_t)(p))

extern "C" {

size_t msmc_relu_bn_workspace(long N, int C) {
    if (!bn_shape_ok(N, C)) return 0;
    const bn_grid gr = bn_slabs(N);
    return (size_t)gr.nblk * (2 * (size_t)C * sizeof(float) + sizeof(int));
}

int msmc_relu_bn_fwd(const void* x, long ldx, const float* gamma, const float* beta, void* y, long ldy, float* mean, float* rstd,
                     float* running_mean, float* running_var, long long* num_batches_tracked, void* workspace,
                     size_t workspace_bytes, long N, int C, float eps, float momentum, int dtype, msmc_stream stream) {
    if (!x || !y || !gamma || !beta || !mean || !rstd || (!running_mean != !running_var)) return MSMC_E_SHAPE;
    if (!rbn_shape_ok(N, C, ldx) || !rbn_shape_ok(N, C, ldy) || N < 2 || dtype < 0 || dtype > 1) return MSMC_E_SHAPE;
    if (!td_aligned(TD_P(x) | TD_P(y) | TD_P(gamma) | TD_P(beta) | TD_P(workspace))) return MSMC_E_SHAPE;
    if (!workspace || workspace_bytes < msmc_relu_bn_workspace(N, C)) return MSMC_E_WORKSPACE;
    const bn_grid gr = bn_slabs(N);
    const dim3 grid((unsigned)gr.nblk, (unsigned)td_chunks(C, td_vec(dtype)));
    float* ws = (float*)workspace;
#define RBN_FWD(T_)                                                                                                          \
    do {                                                                                                                     \
        MSMC_LAUNCH((rbn_stats_kernel<T_>), grid, dim3(256), 0, (msmc_stream_t)stream, (const T_*)x, ldx, ws, N, C, gr.slab, gr.nblk); \
        int rc = msmc_check_launch();                                                                                        \
        if (rc) return rc;                                                                                                   \
        MSMC_LAUNCH((rbn_norm_kernel<T_>), grid, dim3(256), 0, (msmc_stream_t)stream, (const T_*)x, ldx, (const float*)ws, gr.nblk, \
                    gamma, beta, (T_*)y, ldy, mean, rstd, running_mean, running_var, num_batches_tracked, N, C, gr.slab, eps,   \
                    momentum);                                                                                               \
    } while (0)
    MSMC_BY_DTYPE(dtype, RBN_FWD);
#undef RBN_FWD
    return msmc_check_launch();
}

int msmc_relu_bn_eval_fwd(const void* x, long ldx, const float* gamma, const float* beta, const float* running_mean,
                          const float* running_var, void* y, long ldy, float* rstd, long N, int C, float eps, int dtype,
                          msmc_stream stream) {
    if (!x || !y || !gamma || !beta || !running_mean || !running_var) return MSMC_E_SHAPE;
    if (!rbn_shape_ok(N, C, ldx) || !rbn_shape_ok(N, C, ldy) || dtype < 0 || dtype > 1) return MSMC_E_SHAPE;
    if (!td_aligned(TD_P(x) | TD_P(y) | TD_P(gamma) | TD_P(beta))) return MSMC_E_SHAPE;
    if (N == 0) return 0;
    const bn_grid gr = bn_stream_slabs(N);
    const dim3 grid((unsigned)gr.nblk, (unsigned)td_chunks(C, td_vec(dtype)));
#define RBN_EVAL(T_)                                                                                                         \
    MSMC_LAUNCH((rbn_norm_kernel<T_>), grid, dim3(256), 0, (msmc_stream_t)stream, (const T_*)x, ldx, (const float*)nullptr, 0,   \
                gamma, beta, (T_*)y, ldy, (float*)nullptr, rstd, (float*)running_mean, (float*)running_var, (long long*)nullptr, \
                N, C, gr.slab, eps, 0.f)
    MSMC_BY_DTYPE(dtype, RBN_EVAL);
#undef RBN_EVAL
    return msmc_check_launch();
}

int msmc_relu_bn_bwd(const void* g, long ldg, const void* x, long ldx, const float* mean, const float* rstd, const float* gamma,
                     void* gx, long ldgx, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, long N, int C,
                     int dtype, msmc_stream stream) {
    if (!g || !x || !mean || !rstd || !gamma || !gx || !dgamma || !dbeta) return MSMC_E_SHAPE;
    if (!rbn_shape_ok(N, C, ldg) || !rbn_shape_ok(N, C, ldx) || !rbn_shape_ok(N, C, ldgx) || N < 2 || dtype < 0 || dtype > 1)
        return MSMC_E_SHAPE;
    if (!td_aligned(TD_P(g) | TD_P(x) | TD_P(gx) | TD_P(mean) | TD_P(rstd) | TD_P(gamma) | TD_P(dgamma) | TD_P(dbeta) | TD_P(workspace)))
        return MSMC_E_SHAPE;
    if (!workspace || workspace_bytes < msmc_relu_bn_workspace(N, C)) return MSMC_E_WORKSPACE;
    const bn_grid gr = bn_slabs(N);
    const dim3 grid((unsigned)gr.nblk, (unsigned)td_chunks(C, td_vec(dtype)));
    float* ws = (float*)workspace;
#define RBN_BWD(T_)                                                                                                          \
    do {                                                                                                                     \
        MSMC_LAUNCH((rbn_bwd_stats_kernel<T_>), grid, dim3(256), 0, (msmc_stream_t)stream, (const T_*)g, ldg, (const T_*)x, ldx, \
                    mean, rstd, ws, N, C, gr.slab);                                                                          \
        int rc = msmc_check_launch();                                                                                        \
        if (rc) return rc;                                                                                                   \
        MSMC_LAUNCH((rbn_bwd_apply_kernel<T_, false>), grid, dim3(256), 0, (msmc_stream_t)stream, (const T_*)g, ldg, (const T_*)x, \
                    ldx, mean, rstd, gamma, (const float*)ws, gr.nblk, (T_*)gx, ldgx, dgamma, dbeta, N, C, gr.slab);         \
    } while (0)
    MSMC_BY_DTYPE(dtype, RBN_BWD);
#undef RBN_BWD
    return msmc_check_launch();
}

int msmc_relu_bn_eval_bwd(const void* g, long ldg, const void* x, long ldx, const float* running_mean, const float* rstd,
                          const float* gamma, void* gx, long ldgx, float* dgamma, float* dbeta, void* workspace,
                          size_t workspace_bytes, long N, int C, int dtype, msmc_stream stream) {
    if (!g || !x || !running_mean || !rstd || !gamma || !gx || (!dgamma != !dbeta)) return MSMC_E_SHAPE;
    if (!rbn_shape_ok(N, C, ldg) || !rbn_shape_ok(N, C, ldx) || !rbn_shape_ok(N, C, ldgx) || dtype < 0 || dtype > 1) return MSMC_E_SHAPE;
    if (!td_aligned(TD_P(g) | TD_P(x) | TD_P(gx) | TD_P(running_mean) | TD_P(rstd) | TD_P(gamma) | TD_P(dgamma) | TD_P(dbeta) | TD_P(workspace)))
        return MSMC_E_SHAPE;
    if (N == 0) return 0;
    if (dgamma && (!workspace || workspace_bytes < msmc_relu_bn_workspace(N, C))) return MSMC_E_WORKSPACE;
    const bn_grid gr = dgamma ? bn_slabs(N) : bn_stream_slabs(N);
    const dim3 grid((unsigned)gr.nblk, (unsigned)td_chunks(C, td_vec(dtype)));
    float* ws = dgamma ? (float*)workspace : nullptr;
#define RBN_EBWD(T_)                                                                                                         \
    do {                                                                                                                     \
        if (ws) {                                                                                                            \
            MSMC_LAUNCH((rbn_bwd_stats_kernel<T_>), grid, dim3(256), 0, (msmc_stream_t)stream, (const T_*)g, ldg, (const T_*)x, ldx, \
                        running_mean, rstd, ws, N, C, gr.slab);                                                              \
            int rc = msmc_check_launch();                                                                                    \
            if (rc) return rc;                                                                                               \
        }                                                                                                                    \
        MSMC_LAUNCH((rbn_bwd_apply_kernel<T_, true>), grid, dim3(256), 0, (msmc_stream_t)stream, (const T_*)g, ldg, (const T_*)x, \
                    ldx, running_mean, rstd, gamma, (const float*)ws, gr.nblk, (T_*)gx, ldgx, dgamma, dbeta, N, C, gr.slab); \
    } while (0)
    MSMC_BY_DTYPE(dtype, RBN_EBWD);
#undef RBN_EBWD
    return msmc_check_launch();
}

// ---- squeeze-excitation ---------------------------------------------------------------------------------------------------
size_t msmc_se_workspace(int B, int T, int C) {
    if (!se_shape_ok(B, T, C)) return 0;
    return (size_t)B * td_max_slabs(T, B, C) * C * sizeof(float);
}

int msmc_se_fwd(const void* x, const void* res, const float* W1, const float* b1, const float* W2, const float* b2, void* y,
                float* gate, float* mean, float* hidden, void* workspace, size_t workspace_bytes, int B, int T, int C, int dtype,
                msmc_stream stream) {
    if (!x || !res || !W1 || !b1 || !W2 || !b2 || !y || !gate || !mean || !hidden) return MSMC_E_SHAPE;
    if (!se_shape_ok(B, T, C) || dtype < 0 || dtype > 1) return MSMC_E_SHAPE;
    if (!td_aligned(TD_P(x) | TD_P(res) | TD_P(y) | TD_P(gate) | TD_P(workspace))) return MSMC_E_SHAPE;
    if (!workspace || workspace_bytes < msmc_se_workspace(B, T, C)) return MSMC_E_WORKSPACE;
    const int nch = td_chunks(C, td_vec(dtype));
    const bn_grid gr = td_slabs(T, B * nch, false), gs = td_slabs(T, B * nch, true);
    float* ws = (float*)workspace;
#define SE_FWD(T_)                                                                                                           \
    do {                                                                                                                     \
        MSMC_LAUNCH((se_sums_kernel<T_, false>), dim3((unsigned)gr.nblk, (unsigned)nch, (unsigned)B), dim3(256), 0,          \
                    (msmc_stream_t)stream, (const T_*)x, (const T_*)nullptr, ws, T, C, (int)gr.slab);                         \
        int rc = msmc_check_launch();                                                                                        \
        if (rc) return rc;                                                                                                   \
        MSMC_LAUNCH(se_gate_kernel, dim3((unsigned)B), dim3(256), 0, (msmc_stream_t)stream, (const float*)ws, gr.nblk, W1, b1, W2, \
                    b2, gate, mean, hidden, T, C);                                                                           \
        rc = msmc_check_launch();                                                                                            \
        if (rc) return rc;                                                                                                   \
        MSMC_LAUNCH((se_scale_kernel<T_, false>), dim3((unsigned)gs.nblk, (unsigned)nch, (unsigned)B), dim3(256), 0,         \
                    (msmc_stream_t)stream, (const T_*)x, (const float*)gate, res, (T_*)y, T, C, (int)gs.slab);                \
    } while (0)
    MSMC_BY_DTYPE(dtype, SE_FWD);
#undef SE_FWD
    return msmc_check_launch();
}

int msmc_se_bwd_gate(const void* g, const void* x, float* dgate, void* workspace, size_t workspace_bytes, int B, int T, int C,
                     int dtype, msmc_stream stream) {
    if (!g || !x || !dgate || !se_shape_ok(B, T, C) || dtype < 0 || dtype > 1) return MSMC_E_SHAPE;
    if (!td_aligned(TD_P(g) | TD_P(x) | TD_P(workspace))) return MSMC_E_SHAPE;
    if (!workspace || workspace_bytes < msmc_se_workspace(B, T, C)) return MSMC_E_WORKSPACE;
    const int nch = td_chunks(C, td_vec(dtype));
    const bn_grid gr = td_slabs(T, B * nch, false);
    float* ws = (float*)workspace;
#define SE_BG(T_)                                                                                                            \
    MSMC_LAUNCH((se_sums_kernel<T_, true>), dim3((unsigned)gr.nblk, (unsigned)nch, (unsigned)B), dim3(256), 0,               \
                (msmc_stream_t)stream, (const T_*)g, (const T_*)x, ws, T, C, (int)gr.slab)
    MSMC_BY_DTYPE(dtype, SE_BG);
#undef SE_BG
    int rc = msmc_check_launch();
    if (rc) return rc;
    MSMC_LAUNCH(se_merge_kernel, dim3((unsigned)((B * C + 255) / 256)), dim3(256), 0, (msmc_stream_t)stream, (const float*)ws, gr.nblk,
                dgate, B, C);
    return msmc_check_launch();
}

int msmc_se_bwd_apply(const void* g, const float* gate, const float* dmean, void* gx, int B, int T, int C, int dtype,
                      msmc_stream stream) {
    if (!g || !gate || !dmean || !gx || !se_shape_ok(B, T, C) || dtype < 0 || dtype > 1) return MSMC_E_SHAPE;
    if (!td_aligned(TD_P(g) | TD_P(gx) | TD_P(gate) | TD_P(dmean))) return MSMC_E_SHAPE;
    const int nch = td_chunks(C, td_vec(dtype));
    const bn_grid gs = td_slabs(T, B * nch, true);
#define SE_BA(T_)                                                                                                            \
    MSMC_LAUNCH((se_scale_kernel<T_, true>), dim3((unsigned)gs.nblk, (unsigned)nch, (unsigned)B), dim3(256), 0,              \
                (msmc_stream_t)stream, (const T_*)g, gate, (const void*)dmean, (T_*)gx, T, C, (int)gs.slab)
    MSMC_BY_DTYPE(dtype, SE_BA);
#undef SE_BA
    return msmc_check_launch();
}

// ---- attentive statistics pooling -----------------------------------------------------------------------------------------
size_t msmc_asp_workspace(int B, int T, int C) {
    if (!asp_shape_ok(B, T, C)) return 0;
    return (size_t)B * td_max_slabs(T, B, C) * 4 * C * sizeof(float);
}

int msmc_asp_fwd(const void* x, const void* a, float* out, float* stats, void* workspace, size_t workspace_bytes, int B, int T,
                 int C, int dtype, msmc_stream stream) {
    if (!x || !a || !out || !stats || !asp_shape_ok(B, T, C) || dtype < 0 || dtype > 1) return MSMC_E_SHAPE;
    if (!td_aligned(TD_P(x) | TD_P(a) | TD_P(workspace))) return MSMC_E_SHAPE;
    if (!workspace || workspace_bytes < msmc_asp_workspace(B, T, C)) return MSMC_E_WORKSPACE;
    const int nch = td_chunks(C, td_vec(dtype));
    const bn_grid gr = td_slabs(T, B * nch, false);
    float* ws = (float*)workspace;
#define ASP_FWD(T_)                                                                                                          \
    MSMC_LAUNCH((asp_part_kernel<T_>), dim3((unsigned)gr.nblk, (unsigned)nch, (unsigned)B), dim3(256), 0, (msmc_stream_t)stream, \
                (const T_*)x, (const T_*)a, ws, T, C, (int)gr.slab)
    MSMC_BY_DTYPE(dtype, ASP_FWD);
#undef ASP_FWD
    int rc = msmc_check_launch();
    if (rc) return rc;
    MSMC_LAUNCH(asp_merge_kernel, dim3((unsigned)((B * C + 255) / 256)), dim3(256), 0, (msmc_stream_t)stream, (const float*)ws, gr.nblk,
                out, stats, B, C);
    return msmc_check_launch();
}

int msmc_asp_bwd(const float* gout, const void* x, const void* a, const float* stats, void* gx, void* ga, int B, int T, int C,
                 int dtype, msmc_stream stream) {
    if (!gout || !x || !a || !stats || !gx || !ga || !asp_shape_ok(B, T, C) || dtype < 0 || dtype > 1) return MSMC_E_SHAPE;
    if (!td_aligned(TD_P(gout) | TD_P(x) | TD_P(a) | TD_P(stats) | TD_P(gx) | TD_P(ga))) return MSMC_E_SHAPE;
    const int nch = td_chunks(C, td_vec(dtype));
    const bn_grid gs = td_slabs(T, B * nch, true);
#define ASP_BWD(T_)                                                                                                          \
    MSMC_LAUNCH((asp_bwd_kernel<T_>), dim3((unsigned)gs.nblk, (unsigned)nch, (unsigned)B), dim3(256), 0, (msmc_stream_t)stream, \
                gout, (const T_*)x, (const T_*)a, stats, (T_*)gx, (T_*)ga, T, C, (int)gs.slab)
    MSMC_BY_DTYPE(dtype, ASP_BWD);
#undef ASP_BWD
    return msmc_check_launch();
}

}  // extern "C"
