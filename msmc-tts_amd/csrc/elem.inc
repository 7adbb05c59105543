// elem.inc -- typed element access, block / wave sums and the dtype dispatch shared by the helper translation units (norm,
// losses, wnorm, optim, tdnn, window) and, through bn_common.inc / conv_common.inc, by their users.  Included after
// <msmc_rt.hpp>; written in that header's vocabulary only, so the same text is the GPU code and the interpreter's.
#pragma once

// ---- one element: fp32, or bf16 bits (unsigned short), as fp32 ---------------------------------------------------------------
// Every access comes as (p) and as (p, i) = element i of p.  The indexed form is the primary one: it forms the address next
// to the access (a store's after its value is computed); with p + i formed at the call the compiler orders the callers otherwise.
MSMC_DEV float el_ld(const float* p, long i) { return p[i]; }
MSMC_DEV float el_ld(const unsigned short* p, long i) { return bf16_bits_to_f32(p[i]); }
MSMC_DEV void el_st(float* p, long i, float v) { p[i] = v; }
MSMC_DEV void el_st(unsigned short* p, long i, float v) { p[i] = f32_to_bf16_bits(v); }
template <typename T> MSMC_DEV float el_ld(const T* p) { return el_ld(p, 0L); }
template <typename T> MSMC_DEV void el_st(T* p, float v) { el_st(p, 0L, v); }
// the store for a dtype known only at run time (0 fp32, otherwise bf16)
MSMC_DEV void el_st_rt(void* dst, int dtype, long i, float v) {
    if (dtype == 0) ((float*)dst)[i] = v;
    else ((unsigned short*)dst)[i] = f32_to_bf16_bits(v);
}

// ---- V consecutive elements as ONE access (aligned to it): fp32 V = 2 / 4 -> 8 / 16 bytes, V = 8 -> two 16-byte accesses;
// bf16 V = 2 / 4 / 8 -> 4 / 8 / 16 bytes; V = 1 is the scalar access.  Any other width does not compile.
// a pair of bf16 in one 32-bit word, the even element in the low half
MSMC_DEV void el_unpack2(unsigned int w, float& lo, float& hi) {
    lo = __uint_as_float(w << 16);
    hi = __uint_as_float(w & 0xffff0000u);
}
MSMC_DEV unsigned int el_pack2(float lo, float hi) { return (unsigned)f32_to_bf16_bits(lo) | ((unsigned)f32_to_bf16_bits(hi) << 16); }
#define EL_WIDTH_OK(V) static_assert(V == 1 || V == 2 || V == 4 || V == 8, "el_ldv / el_stv: 1, 2, 4 or 8 elements")
template <int V> MSMC_DEV void el_ldv(const float* p, long i, float (&o)[V]) {
    EL_WIDTH_OK(V);
    if constexpr (V == 1) {
        o[0] = p[i];
    } else if constexpr (V == 2) {
        const f32x2 t = *(const f32x2*)(p + i);
        o[0] = t[0];
        o[1] = t[1];
    } else {
#pragma unroll
        for (int h = 0; h < V / 4; ++h) {
            const f32x4 t = *(const f32x4*)(p + i + 4 * h);
#pragma unroll
            for (int q = 0; q < 4; ++q) o[4 * h + q] = t[q];
        }
    }
}
template <int V> MSMC_DEV void el_ldv(const unsigned short* p, long i, float (&o)[V]) {
    EL_WIDTH_OK(V);
    if constexpr (V == 1) {
        o[0] = bf16_bits_to_f32(p[i]);
    } else if constexpr (V == 2) {
        const unsigned int t = *(const unsigned int*)(p + i);
        el_unpack2(t, o[0], o[1]);
    } else if constexpr (V == 4) {
        const u32x2 t = *(const u32x2*)(p + i);
#pragma unroll
        for (int h = 0; h < 2; ++h) el_unpack2(t[h], o[2 * h], o[2 * h + 1]);
    } else {
        const u32x4 t = *(const u32x4*)(p + i);
#pragma unroll
        for (int h = 0; h < 4; ++h) el_unpack2(t[h], o[2 * h], o[2 * h + 1]);
    }
}
template <int V> MSMC_DEV void el_stv(float* p, long i, const float (&v)[V]) {
    EL_WIDTH_OK(V);
    if constexpr (V == 1) {
        p[i] = v[0];
    } else if constexpr (V == 2) {
        const f32x2 t = {v[0], v[1]};
        *(f32x2*)(p + i) = t;
    } else {
#pragma unroll
        for (int h = 0; h < V / 4; ++h) {
            f32x4 t;
#pragma unroll
            for (int q = 0; q < 4; ++q) t[q] = v[4 * h + q];
            *(f32x4*)(p + i + 4 * h) = t;
        }
    }
}
template <int V> MSMC_DEV void el_stv(unsigned short* p, long i, const float (&v)[V]) {
    EL_WIDTH_OK(V);
    if constexpr (V == 1) {
        p[i] = f32_to_bf16_bits(v[0]);
    } else if constexpr (V == 2) {
        *(unsigned int*)(p + i) = el_pack2(v[0], v[1]);
    } else if constexpr (V == 4) {
        u32x2 t;
#pragma unroll
        for (int h = 0; h < 2; ++h) t[h] = el_pack2(v[2 * h], v[2 * h + 1]);
        *(u32x2*)(p + i) = t;
    } else {
        u32x4 t;
#pragma unroll
        for (int h = 0; h < 4; ++h) t[h] = el_pack2(v[2 * h], v[2 * h + 1]);
        *(u32x4*)(p + i) = t;
    }
}
#undef EL_WIDTH_OK
template <int V, typename T> MSMC_DEV void el_ldv(const T* p, float (&o)[V]) { el_ldv<V>(p, 0L, o); }
template <int V, typename T> MSMC_DEV void el_stv(T* p, const float (&v)[V]) { el_stv<V>(p, 0L, v); }

// ---- sums ----------------------------------------------------------------------------------------------------------------------
// sum over the 256 work-items of a workgroup through red[256], a tree in a fixed order; every work-item returns the total.
// RESYNC: a closing barrier, so that red may be written again at once (a second call, or the caller's own use of it).
template <bool RESYNC> MSMC_DEV float block_tree_sum(float v, float* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    const float r = red[0];
    if (RESYNC) __syncthreads();
    return r;
}
// sum over the 64 lanes by the xor butterfly, masks 32 .. 1; every lane ends with the total.  NOT wave_sum of msmc_rt.hpp: that
// one adds in another order (DPP steps inside a row first, then the row and half swaps) and gives other bits -- results that are
// compared bit for bit between runs or builds keep the sum they were written with.
MSMC_DEV float wave_xor_sum(float v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v = v + wave_xor(v, m);
    return v;
}

// ---- host: one instantiation per element type --------------------------------------------------------------------------------
// GO is a function-like macro defined next to the launch (the kernel's type is already substituted when MSMC_LAUNCH turns the
// kernel expression into the launch log's name).  dtype 0 -> GO(float), 1 -> GO(unsigned short), anything else is refused.
#define MSMC_BY_DTYPE(dtype, GO)                        \
    do {                                                \
        if ((dtype) == 0) GO(float);                    \
        else if ((dtype) == 1) GO(unsigned short);      \
        else return MSMC_E_SHAPE;                       \
    } while (0)
// (element type, type of the second operand): fp32 / fp32, bf16 / fp32 when other == 0, bf16 / bf16; the caller has checked both
#define MSMC_BY_DTYPE2(dtype, other, GO)                        \
    do {                                                        \
        if ((dtype) == 0) GO(float, float);                     \
        else if ((other) == 0) GO(unsigned short, float);       \
        else GO(unsigned short, unsigned short);                \
    } while (0)
// every address or-ed into `addrs` is aligned for a four-element access of the dtype: 16 bytes of fp32, 8 bytes of bf16
static inline bool msmc_aligned4(size_t addrs, int dtype) { return (addrs & (dtype == 0 ? 15 : 7)) == 0; }
