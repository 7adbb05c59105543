// unit_ce.hip -- the unit predictor's loss and its label decoding, for gfx950: length-masked cross-entropy of logits [B][T][ld]
// (the first K columns of a row are the classes; K = 100 ... 2000 k-means units) against stored labels, its gradient, and the
// arg-max alone.  Host side: msmctts_amd/hip/unit_ce.py (masked_cross_entropy, unit_argmax).  The stock chain this replaces
// (cross_entropy(reduction='none'), masked_fill, sum, divide) stores an [N][K] fp32 log-probability tensor and its gradient;
// here the forward reads the logits once and stores 4 (+ 8) bytes per row, the backward reads them once more and writes the
// gradient.
//
// Rows.  Row n = (b, t) is VALID when t < lengths[b]; the logits of any other row are never read.  A valid row whose target is
// outside [0, K) is IGNORED: no loss, zero gradient (its lse and arg-max are still stored).  The denominator is the sum of the
// lengths as they are given (the reference's), whatever the targets.
//
// Work split (all three kernels).  A WAVE PER ROW: at K = 100 ... 2000 a row is 0.4 ... 8 KB, one to eight 1 KB wave loads, and the
// three per-row results merge through the wave without LDS.  A workgroup is 256 work-items = UC_ROWS = 4 rows; the flattened rows
// are cut into groups of 4 and the grid is the number of groups, at most 8 workgroups per CU (2048: the usual bound of a
// streaming kernel, guide section 6 rule 11) -- beyond that a workgroup strides over the groups.  The kernels use no LDS beyond
// 32 bytes and few registers, so 8 workgroups = 32 waves per CU are resident, each with up to UC_UNROLL = 4 loads of 1 KB in
// flight.  Vector path: 16-byte loads and stores (V = 4 fp32 / 8 bf16 elements) where ld % V == 0 and the base addresses are
// 16-byte aligned; otherwise the scalar path (V = 1), the same code.
//
// ORDER of a row's scan (uc_scan), restated by tests/_unitcecases.py for its error bound.  Lane l owns the vectors l, l + 64,
// ... of the K / V whole vectors of the row, then -- as a vector of one -- element V (K / V) + l of the K % V left over.  Running
// state per lane: maximum m (-inf), sum s (0), arg-max a.  Per vector, in ascending order: its maximum is found first (ascending
// scan, strict >, so the lowest index wins a tie); if it exceeds m then s <- s expf(m - max), m <- max, a <- its index; then
// s <- ((s + expf(x_0 - m)) + expf(x_1 - m)) + ...  The 64 lanes merge by the xor butterfly, masks 32 ... 1: M = max(m, m'),
// s <- s e + s' e' with e = 1 where m == M and expf(m - M) otherwise; the larger maximum keeps its index, the lower index on a
// tie.  lse = m + logf(s), row loss = lse - x[target].  Only comparisons decide the arg-max: it is exact.
//
// msmc_unit_ce_fwd, launch 1 (uc_fwd_kernel): wave w of a workgroup adds the losses of its rows (((0 + l_0) + l_1) + ...) in
// ascending group order and counts pred == target; the workgroup's partial is ((p_0 + p_1) + p_2) + p_3 over its waves.  Launch
// 2 (uc_final_kernel, one wave): lane l adds the partials l, l + 64, ... in ascending order, the lanes merge by the xor
// butterfly (wave_xor_sum); the counts likewise, in integers.  tot = the sum of the lengths (64-bit integer, exact);
// out[0] = sum / (float)tot, out[1] = 1 / (float)tot, correct = the count.  tot <= 0 (no valid row can count): out[0] = out[1] = 0
// -- a defined zero loss and zero gradient where the stock chain divides 0 by 0.  No floating-point atomics: within one build,
// the same inputs give the same bits.
//
// msmc_unit_ce_bwd (uc_bwd_kernel): glogits[n][k] = (expf(x_k - lse[n]) - [k == target[n]]) * (gout[0] * out[1]) for k < K on
// the valid, not ignored rows; exact +0 in the columns K ... ld - 1, on padded and on ignored rows.  Every element of glogits is
// written exactly once.
//
// Workspace of the forward: G floats of loss partials (rounded up to 16 bytes), then G ints of counts, G = the forward's grid.
#include <msmc_rt.hpp>
#include <msmc_hip.h>

#include "elem.inc"

#define UC_WG 256
#define UC_ROWS (UC_WG / MSMC_WAVE)      // rows of a group: one per wave
#define UC_UNROLL 4                      // vectors a lane has in flight
#define UC_NONE 0x7fffffff               // arg-max of a lane that saw no element

MSMC_DEV long uc_len(const void* len, int is64, long b) {
    return is64 ? (long)((const long long*)len)[b] : (long)((const int*)len)[b];
}
MSMC_DEV float uc_neg_inf() { return __uint_as_float(0xff800000u); }

struct uc_state {
    float m, s;
    int a;
};

// one vector of the lane's share: the elements x[0 .. n) are columns k0 .. k0 + n - 1
template <int V, bool LSE> MSMC_DEV void uc_take(uc_state& st, const float (&x)[V], int n, int k0) {
    float vm = x[0];
    int va = 0;
#pragma unroll
    for (int i = 1; i < V; ++i)
        if (i < n && x[i] > vm) {
            vm = x[i];
            va = i;
        }
    if (vm > st.m) {
        if (LSE) st.s = st.s * expf(st.m - vm);
        st.m = vm;
        st.a = k0 + va;
    }
    if (LSE) {
#pragma unroll
        for (int i = 0; i < V; ++i)
            if (i < n) st.s = st.s + expf(x[i] - st.m);
    }
}

// the scan of one row by the calling wave (see ORDER); every lane returns the row's maximum, sum and arg-max
template <typename T, int V, bool LSE> MSMC_DEV uc_state uc_scan(const T* __restrict__ row, int K, int lane) {
    uc_state st;
    st.m = uc_neg_inf();
    st.s = 0.f;
    st.a = UC_NONE;
    const int nv = K / V;
    for (int v0 = lane; v0 < nv; v0 += MSMC_WAVE * UC_UNROLL) {
        float x[UC_UNROLL][V];
#pragma unroll
        for (int j = 0; j < UC_UNROLL; ++j) {
            const int v = v0 + j * MSMC_WAVE;
            if (v < nv) el_ldv<V>(row, (long)v * V, x[j]);
        }
#pragma unroll
        for (int j = 0; j < UC_UNROLL; ++j) {
            const int v = v0 + j * MSMC_WAVE;
            if (v < nv) uc_take<V, LSE>(st, x[j], V, v * V);
        }
    }
    if (V > 1 && nv * V + lane < K) {
        float x[V];
        x[0] = el_ld(row, (long)(nv * V + lane));
        uc_take<V, LSE>(st, x, 1, nv * V + lane);
    }
#pragma unroll
    for (int mask = 32; mask > 0; mask >>= 1) {
        const float m2 = wave_xor(st.m, mask);
        const int a2 = wave_xor(st.a, mask);
        const float M = m2 > st.m ? m2 : st.m;
        if (LSE) {
            const float s2 = wave_xor(st.s, mask);
            const float e1 = st.m == M ? 1.f : expf(st.m - M), e2 = m2 == M ? 1.f : expf(m2 - M);
            st.s = st.s * e1 + s2 * e2;
        }
        if (m2 > st.m || (m2 == st.m && a2 < st.a)) st.a = a2;
        st.m = M;
    }
    return st;
}

// WITH_LOSS: the forward's first launch; otherwise the arg-max alone (target, lse and the partials are not touched)
template <typename T, int V, bool WITH_LOSS>
__global__ __launch_bounds__(UC_WG) void uc_fwd_kernel(const T* __restrict__ logits, const int64_t* __restrict__ target,
                                                      const void* __restrict__ len, int is64, float* __restrict__ lse,
                                                      int64_t* __restrict__ pred, float* __restrict__ part, int* __restrict__ cnt,
                                                      long N, int Tn, int K, long ld, long groups) {
    __shared__ float sl[UC_ROWS];
    __shared__ int sc[UC_ROWS];
    const int lane = threadIdx.x & (MSMC_WAVE - 1), wave = threadIdx.x / MSMC_WAVE;
    float acc = 0.f;
    int hit = 0;
    for (long g = blockIdx.x; g < groups; g += gridDim.x) {
        const long n = g * UC_ROWS + wave;
        if (n >= N) continue;                                        // (the same in every lane of the wave)
        const long b = n / Tn;
        if (n - b * Tn >= uc_len(len, is64, b)) {
            if (lane == 0) {
                if (WITH_LOSS) lse[n] = 0.f;
                if (pred) pred[n] = -1;
            }
            continue;
        }
        const T* row = logits + (size_t)n * ld;
        const uc_state st = uc_scan<T, V, WITH_LOSS>(row, K, lane);
        if (WITH_LOSS) {
            const float l = st.m + logf(st.s);
            const int64_t tg = target[n];
            const bool counts = tg >= 0 && tg < K;
            if (counts) {
                acc = acc + (l - el_ld(row, (long)tg));
                if ((int64_t)st.a == tg) ++hit;
            }
            if (lane == 0) lse[n] = l;
        }
        if (lane == 0 && pred) pred[n] = st.a;
    }
    if (WITH_LOSS) {
        if (lane == 0) {
            sl[wave] = acc;
            sc[wave] = hit;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            float p = sl[0];
            int c = sc[0];
            for (int w = 1; w < UC_ROWS; ++w) {
                p = p + sl[w];
                c += sc[w];
            }
            part[blockIdx.x] = p;
            cnt[blockIdx.x] = c;
        }
    }
}

__global__ __launch_bounds__(MSMC_WAVE) void uc_final_kernel(const float* __restrict__ part, const int* __restrict__ cnt, int nparts,
                                                            const void* __restrict__ len, int is64, int B, float* __restrict__ out,
                                                            int64_t* __restrict__ correct) {
    const int lane = threadIdx.x;
    float s = 0.f;
    int c = 0;
    for (int k = lane; k < nparts; k += MSMC_WAVE) {
        s = s + part[k];
        c += cnt[k];
    }
    s = wave_xor_sum(s);
#pragma unroll
    for (int mask = 32; mask > 0; mask >>= 1) c += wave_xor(c, mask);
    if (lane == 0) {
        long tot = 0;                                                // (the reference sums the lengths as they are: no clamp to T)
        for (int b = 0; b < B; ++b) tot += uc_len(len, is64, b);
        out[0] = tot > 0 ? s / (float)tot : 0.f;
        out[1] = tot > 0 ? 1.f / (float)tot : 0.f;
        if (correct) correct[0] = c;
    }
}

template <typename T, int V>
__global__ __launch_bounds__(UC_WG) void uc_bwd_kernel(const T* __restrict__ logits, const int64_t* __restrict__ target,
                                                      const void* __restrict__ len, int is64, const float* __restrict__ lse,
                                                      const float* __restrict__ out, const float* __restrict__ gout,
                                                      T* __restrict__ glogits, long N, int Tn, int K, long ld, long groups) {
    const int lane = threadIdx.x & (MSMC_WAVE - 1), wave = threadIdx.x / MSMC_WAVE;
    const float scale = gout[0] * out[1];
    const int nv = (int)(ld / V);                                    // (V divides ld on the vector path)
    for (long g = blockIdx.x; g < groups; g += gridDim.x) {
        const long n = g * UC_ROWS + wave;
        if (n >= N) continue;
        const long b = n / Tn;
        int64_t tg = -1;
        if (n - b * Tn < uc_len(len, is64, b)) tg = target[n];
        const bool live = tg >= 0 && tg < K;                         // valid and not ignored
        const T* row = logits + (size_t)n * ld;
        T* grow = glogits + (size_t)n * ld;
        const float l = live ? lse[n] : 0.f;
        for (int v0 = lane; v0 < nv; v0 += MSMC_WAVE * UC_UNROLL) {
            float x[UC_UNROLL][V];
            if (live) {
#pragma unroll
                for (int j = 0; j < UC_UNROLL; ++j) {
                    const int v = v0 + j * MSMC_WAVE;
                    if (v < nv && v * V < K) el_ldv<V>(row, (long)v * V, x[j]);
                }
            }
#pragma unroll
            for (int j = 0; j < UC_UNROLL; ++j) {
                const int v = v0 + j * MSMC_WAVE;
                if (v >= nv) continue;
                float o[V];
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    const int k = v * V + i;
                    o[i] = 0.f;
                    if (live && k < K) o[i] = (expf(x[j][i] - l) - (k == (int)tg ? 1.f : 0.f)) * scale;
                }
                el_stv<V>(grow, (long)v * V, o);
            }
        }
    }
}

static inline size_t uc_round16(size_t bytes) { return (bytes + 15) / 16 * 16; }

struct uc_plan {
    long N, groups, grid;
    size_t cnt, bytes;               // offset of the counts, bytes of the forward's workspace
};

// false for the sizes no kernel here takes
static bool uc_make_plan(int B, int T, uc_plan& pl) {
    if (B < 1 || T < 1 || (long)B * T > 0x7fffffffL) return false;
    pl.N = (long)B * T;
    pl.groups = (pl.N + UC_ROWS - 1) / UC_ROWS;
    pl.grid = pl.groups < 8L * MSMC_NUM_CU ? pl.groups : 8L * MSMC_NUM_CU;
    pl.cnt = uc_round16((size_t)pl.grid * sizeof(float));
    pl.bytes = pl.cnt + uc_round16((size_t)pl.grid * sizeof(int));
    return true;
}

static inline bool uc_takes(const void* logits, const void* lengths, int dtype, int K, int ld) {
    return logits && lengths && (dtype == 0 || dtype == 1) && K >= 1 && K <= ld;
}
// the 16-byte path: whole vectors per row and every row start aligned
static inline bool uc_vector(size_t addrs, int dtype, int ld) { return (addrs & 15) == 0 && ld % (dtype == 0 ? 4 : 8) == 0; }

#define UC_BY_PATH(dtype, vec, GO)                      \
    do {                                                \
        if ((dtype) == 0) {                             \
            if (vec) GO(float, 4);                      \
            else GO(float, 1);                          \
        } else {                                        \
            if (vec) GO(unsigned short, 8);             \
            else GO(unsigned short, 1);                 \
        }                                               \
    } while (0)

extern "C" {

size_t msmc_unit_ce_workspace(int B, int T) {
    uc_plan pl;
    return uc_make_plan(B, T, pl) ? pl.bytes : 0;
}

int msmc_unit_ce_fwd(const void* logits, int dtype, const int64_t* target, const void* lengths, int len_is_64, float* lse, int64_t* pred,
                     float* out, int64_t* correct, void* workspace, size_t workspace_bytes, int B, int T, int K, int ld,
                     msmc_stream stream) {
    uc_plan pl;
    if (!uc_takes(logits, lengths, dtype, K, ld) || !target || !lse || !out || !uc_make_plan(B, T, pl)) return MSMC_E_SHAPE;
    if (!workspace || ((uintptr_t)workspace & 15) != 0 || workspace_bytes < pl.bytes) return MSMC_E_WORKSPACE;
    msmc_stream_t st = (msmc_stream_t)stream;
    float* part = (float*)workspace;
    int* cnt = (int*)((char*)workspace + pl.cnt);
    const bool vec = uc_vector((uintptr_t)logits, dtype, ld);
#define UC_FWD(T_, V_)                                                                                                              \
    MSMC_LAUNCH((uc_fwd_kernel<T_, V_, true>), dim3((unsigned)pl.grid), dim3(UC_WG), 0, st, (const T_*)logits, target, lengths, \
                len_is_64, lse, pred, part, cnt, pl.N, T, K, (long)ld, pl.groups)
    UC_BY_PATH(dtype, vec, UC_FWD);
#undef UC_FWD
    const int rc = msmc_check_launch();
    if (rc) return rc;
    MSMC_LAUNCH(uc_final_kernel, dim3(1), dim3(MSMC_WAVE), 0, st, (const float*)part, (const int*)cnt, (int)pl.grid, lengths, len_is_64, B,
                out, correct);
    return msmc_check_launch();
}

int msmc_unit_ce_bwd(const void* logits, int dtype, const int64_t* target, const void* lengths, int len_is_64, const float* lse,
                     const float* out, const float* gout, void* glogits, int B, int T, int K, int ld, msmc_stream stream) {
    uc_plan pl;
    if (!uc_takes(logits, lengths, dtype, K, ld) || !target || !lse || !out || !gout || !glogits || !uc_make_plan(B, T, pl))
        return MSMC_E_SHAPE;
    const bool vec = uc_vector((uintptr_t)logits | (uintptr_t)glogits, dtype, ld);
#define UC_BWD(T_, V_)                                                                                                            \
    MSMC_LAUNCH((uc_bwd_kernel<T_, V_>), dim3((unsigned)pl.grid), dim3(UC_WG), 0, (msmc_stream_t)stream, (const T_*)logits, target, \
                lengths, len_is_64, lse, out, gout, (T_*)glogits, pl.N, T, K, (long)ld, pl.groups)
    UC_BY_PATH(dtype, vec, UC_BWD);
#undef UC_BWD
    return msmc_check_launch();
}

int msmc_unit_argmax(const void* logits, int dtype, const void* lengths, int len_is_64, int64_t* pred, int B, int T, int K, int ld,
                     msmc_stream stream) {
    uc_plan pl;
    if (!uc_takes(logits, lengths, dtype, K, ld) || !pred || !uc_make_plan(B, T, pl)) return MSMC_E_SHAPE;
    const bool vec = uc_vector((uintptr_t)logits, dtype, ld);
#define UC_ARG(T_, V_)                                                                                                              \
    MSMC_LAUNCH((uc_fwd_kernel<T_, V_, false>), dim3((unsigned)pl.grid), dim3(UC_WG), 0, (msmc_stream_t)stream, (const T_*)logits, \
                (const int64_t*)nullptr, lengths, len_is_64, (float*)nullptr, pred, (float*)nullptr, (int*)nullptr, pl.N, T, K,     \
                (long)ld, pl.groups)
    UC_BY_PATH(dtype, vec, UC_ARG);
#undef UC_ARG
    return msmc_check_launch();
}

}  // extern "C"
