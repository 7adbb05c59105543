// spectral.hip -- STFT framing and magnitude / log / mel glue kernels for gfx950.
//
// The DFT itself and the mel projections run as one-tap channels-last "convolutions" (plain GEMMs) on the
// fp32 matrix cores through msmc_conv_gather; these kernels are the memory-bound pieces around them:
// reflect-padded framing and its overlap-add adjoint, magnitude, the MRD two-channel image with the
// transposition to the channels-last [B][F][T][2] layout the discriminator stack consumes, and log-clamp.
// Replaces torch.stft + glue of TorchSTFT.transform (reference msmctts/utils/audio.py:398-419),
// MelScale.forward (:348-376) and MelLoss.mel_spectrogram (reference criterions/stft_loss.py:76-108).
#include <msmc_rt.hpp>
#include <msmc_hip.h>

MSMC_DEV int sp_reflect(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return i;
}

MSMC_DEV void stft_frames_fwd_body(const float* __restrict__ x, float* __restrict__ fr, int L,
                                                             int T, int n_fft, int NP, int hop, int pad, long total, int bid, int nb) {
    for (long e = (long)bid * 256 + threadIdx.x; e < total; e += (long)nb * 256) {
        const int j = (int)(e % NP);
        const long r = e / NP;
        const int t = (int)(r % T);
        const long b = r / T;
        float v = 0.f;
        if (j < n_fft) v = x[b * L + sp_reflect(t * hop + j - pad, L)];
        fr[e] = v;
    }
}
__global__ __launch_bounds__(256) void stft_frames_fwd_kernel(const float* __restrict__ x, float* __restrict__ fr, int L,
                                                             int T, int n_fft, int NP, int hop, int pad, long total) {
    stft_frames_fwd_body(x, fr, L, T, n_fft, NP, hop, pad, total, (int)blockIdx.x, (int)gridDim.x);
}

// gx[b][l]: frames read padded position p = t*hop + j; sample l is read at p = l + pad and, through the
// reflection, at p = pad - l (l >= 1, left border) and p = 2(L-1) - l + pad (l <= L-2, right border).
MSMC_DEV void stft_frames_bwd_body(const float* __restrict__ gfr, float* __restrict__ gx,
                                                             int L, int T, int n_fft, int NP, int hop, int pad,
                                                             long total, int bid, int nb) {
    const int Lp = (T - 1) * hop + n_fft;           // padded positions actually covered by frames
    for (long e = (long)bid * 256 + threadIdx.x; e < total; e += (long)nb * 256) {
        const int l = (int)(e % L);
        const long b = e / L;
        int ps[3], np = 0;
        ps[np++] = l + pad;
        if (l >= 1 && l <= pad) ps[np++] = pad - l;
        if (l <= L - 2 && 2 * (L - 1) - l + pad < Lp) ps[np++] = 2 * (L - 1) - l + pad;
        float s = 0.f;
        for (int q = 0; q < np; ++q) {
            const int p = ps[q];
            if (p < 0 || p >= Lp) continue;
            int t_hi = p / hop;
            if (t_hi > T - 1) t_hi = T - 1;
            int t_lo = (p - n_fft + hop) / hop;      // ceil((p - n_fft + 1) / hop)
            if (p - n_fft + 1 <= 0) t_lo = 0;
            for (int t = t_lo; t <= t_hi; ++t) {
                const int j = p - t * hop;
                if (j >= 0 && j < n_fft) s = s + gfr[(b * T + t) * NP + j];
            }
        }
        gx[e] = s;
    }
}
__global__ __launch_bounds__(256) void stft_frames_bwd_kernel(const float* __restrict__ gfr, float* __restrict__ gx,
                                                             int L, int T, int n_fft, int NP, int hop, int pad,
                                                             long total) {
    stft_frames_bwd_body(gfr, gx, L, T, n_fft, NP, hop, pad, total, (int)blockIdx.x, (int)gridDim.x);
}

MSMC_DEV void spec_mag_fwd_body(const float* __restrict__ spec, float* __restrict__ mag, int F,
                                                          int CP, int FP, float lo, int clamp_mode, long total, int bid, int nb) {
    for (long e = (long)bid * 256 + threadIdx.x; e < total; e += (long)nb * 256) {
        const int f = (int)(e % FP);
        const long r = e / FP;
        float v = 0.f;
        if (f < F) {
            const float re = spec[r * CP + f], im = spec[r * CP + F + f];
            float s = re * re + im * im;
            s = clamp_mode ? (s < lo ? lo : s) : (s + lo);
            v = sqrtf(s);
        }
        mag[e] = v;
    }
}
__global__ __launch_bounds__(256) void spec_mag_fwd_kernel(const float* __restrict__ spec, float* __restrict__ mag, int F,
                                                          int CP, int FP, float lo, int clamp_mode, long total) {
    spec_mag_fwd_body(spec, mag, F, CP, FP, lo, clamp_mode, total, (int)blockIdx.x, (int)gridDim.x);
}

MSMC_DEV void spec_mag_bwd_body(const float* __restrict__ spec, const float* __restrict__ mag,
                                                          const float* __restrict__ gmag, float* __restrict__ gspec,
                                                          int F, int CP, int FP, float lo, int clamp_mode, long total, int bid, int nb) {
    for (long e = (long)bid * 256 + threadIdx.x; e < total; e += (long)nb * 256) {
        const int c = (int)(e % CP);
        const long r = e / CP;
        float g = 0.f;
        if (c < 2 * F) {
            const int f = c < F ? c : c - F;
            const float re = spec[r * CP + f], im = spec[r * CP + F + f];
            const float s = re * re + im * im;
            if (!clamp_mode || s > lo) g = gmag[r * FP + f] * (c < F ? re : im) / mag[r * FP + f];
        }
        gspec[e] = g;
    }
}
__global__ __launch_bounds__(256) void spec_mag_bwd_kernel(const float* __restrict__ spec, const float* __restrict__ mag,
                                                          const float* __restrict__ gmag, float* __restrict__ gspec,
                                                          int F, int CP, int FP, float lo, int clamp_mode, long total) {
    spec_mag_bwd_body(spec, mag, gmag, gspec, F, CP, FP, lo, clamp_mode, total, (int)blockIdx.x, (int)gridDim.x);
}

// img[b][f][t][0..1] <- mel[(b*T + t)][f]   (transposed write; reads are the strided side, tiny tensors)
// (image element type O: float, or bf16 bits when the discriminator stack computes in bf16 -- no separate cast launch)
MSMC_DEV void sp_store2(float* p, float a, float b) { f32x2 o = {a, b}; *(f32x2*)p = o; }
MSMC_DEV void sp_store2(unsigned short* p, float a, float b) {
    *(unsigned int*)p = (unsigned int)f32_to_bf16_bits(a) | ((unsigned int)f32_to_bf16_bits(b) << 16);
}
MSMC_DEV void sp_load2(const float* p, float& a, float& b) { const f32x2 v = *(const f32x2*)p; a = v[0]; b = v[1]; }
MSMC_DEV void sp_load2(const unsigned short* p, float& a, float& b) {
    const unsigned int v = *(const unsigned int*)p;
    a = __uint_as_float(v << 16);
    b = __uint_as_float(v & 0xffff0000u);
}
template <typename O>
MSMC_DEV void mrd_image_fwd_body(const float* __restrict__ mel, O* __restrict__ img, int T,
                                                           int F, int FP, long total, int bid, int nb) {
    for (long e = (long)bid * 256 + threadIdx.x; e < total; e += (long)nb * 256) {
        const int t = (int)(e % T);
        long r = e / T;
        const int f = (int)(r % F);
        const long b = r / F;
        const float m = mel[(b * T + t) * FP + f];
        float lg = (20.f * log10f(m) - 20.f + 100.f) / 100.f;
        lg = lg < 0.f ? 0.f : (lg > 1.f ? 1.f : lg);
        sp_store2(img + e * 2, m, lg);
    }
}
template <typename O>
__global__ __launch_bounds__(256) void mrd_image_fwd_kernel(const float* __restrict__ mel, O* __restrict__ img, int T,
                                                           int F, int FP, long total) {
    mrd_image_fwd_body<O>(mel, img, T, F, FP, total, (int)blockIdx.x, (int)gridDim.x);
}

template <typename O>
MSMC_DEV void mrd_image_bwd_body(const float* __restrict__ mel, const O* __restrict__ gimg,
                                                           float* __restrict__ gmel, int T, int F, int FP, long total, int bid, int nb) {
    for (long e = (long)bid * 256 + threadIdx.x; e < total; e += (long)nb * 256) {
        const int f = (int)(e % FP);
        const long r = e / FP;              // b*T + t
        const int t = (int)(r % T);
        const long b = r / T;
        float g = 0.f;
        if (f < F) {
            const float m = mel[e];
            float g0, g1;
            sp_load2(gimg + (((b * F + f) * (long)T) + t) * 2, g0, g1);
            const float lg = (20.f * log10f(m) - 20.f + 100.f) / 100.f;
            g = g0;
            if (lg > 0.f && lg < 1.f) g = g + g1 * (0.2f / (2.302585092994046f * m));
        }
        gmel[e] = g;
    }
}
template <typename O>
__global__ __launch_bounds__(256) void mrd_image_bwd_kernel(const float* __restrict__ mel, const O* __restrict__ gimg,
                                                           float* __restrict__ gmel, int T, int F, int FP, long total) {
    mrd_image_bwd_body<O>(mel, gimg, gmel, T, F, FP, total, (int)blockIdx.x, (int)gridDim.x);
}

// Single-channel image [B][F][T][1] (the 'linear' / 'log' domains of the resolution discriminators, reference audio.py:410-415):
// CH = 0 the magnitude, CH = 1 the normalised log-magnitude, each by the expression of the same channel of mrd_image_fwd_body --
// the value is that channel bit for bit, and the other channel is neither computed nor stored.  With one channel a lane that owned
// one (f, t) would store 2 (bf16) or 4 bytes; here a lane owns FOUR consecutive elements of the flat image (consecutive t, across a
// row end where T is no multiple of 4) and stores them as one 8-byte (bf16) or 16-byte (fp32) vector.  An image whose base is not
// aligned to the run, and the last partial run, are stored element by element.
MSMC_DEV void sp_store4(float* p, const float (&v)[4]) { f32x4 o = {v[0], v[1], v[2], v[3]}; *(f32x4*)p = o; }
MSMC_DEV void sp_store4(unsigned short* p, const float (&v)[4]) {
    u32x2 o = {(unsigned int)f32_to_bf16_bits(v[0]) | ((unsigned int)f32_to_bf16_bits(v[1]) << 16),
               (unsigned int)f32_to_bf16_bits(v[2]) | ((unsigned int)f32_to_bf16_bits(v[3]) << 16)};
    *(u32x2*)p = o;
}
MSMC_DEV void sp_store1(float* p, float a) { *p = a; }
MSMC_DEV void sp_store1(unsigned short* p, float a) { *p = f32_to_bf16_bits(a); }
MSMC_DEV float sp_load1(const float* p) { return *p; }
MSMC_DEV float sp_load1(const unsigned short* p) { return bf16_bits_to_f32(*p); }
template <typename O, int CH>
MSMC_DEV void mrd_image1_fwd_body(const float* __restrict__ mel, O* __restrict__ img, int T,
                                                            int F, int FP, long total, int bid, int nb) {
    const bool vec = ((size_t)img % (4 * sizeof(O))) == 0;
    const long nrun = (total + 3) / 4;
    for (long q = (long)bid * 256 + threadIdx.x; q < nrun; q += (long)nb * 256) {
        const long e0 = q * 4;
        int t = (int)(e0 % T);
        long r = e0 / T;
        int f = (int)(r % F);
        long b = r / F;
        float m4[4], v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {                   // (the four strided reads leave together)
            m4[u] = e0 + u < total ? mel[(b * T + t) * FP + f] : 1.f;
            if (++t == T) {
                t = 0;
                if (++f == F) { f = 0; ++b; }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float m = m4[u];
            if (CH == 0) {
                v[u] = m;
            } else {
                float lg = (20.f * log10f(m) - 20.f + 100.f) / 100.f;
                lg = lg < 0.f ? 0.f : (lg > 1.f ? 1.f : lg);
                v[u] = lg;
            }
        }
        if (vec && e0 + 4 <= total) {
            sp_store4(img + e0, v);
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (e0 + u < total) sp_store1(img + e0 + u, v[u]);
        }
    }
}
template <typename O, int CH>
__global__ __launch_bounds__(256) void mrd_image1_fwd_kernel(const float* __restrict__ mel, O* __restrict__ img, int T,
                                                            int F, int FP, long total) {
    mrd_image1_fwd_body<O, CH>(mel, img, T, F, FP, total, (int)blockIdx.x, (int)gridDim.x);
}

// gmel[b][t][f] from the single-channel image gradient gimg[b][f][t]: CH = 0 the gradient itself, CH = 1 times d lg / d m inside
// the clamp and zero where the clamp is active (as channel 1 of mrd_image_bwd_body); columns F..FP-1 zero.  A lane owns four
// consecutive f of one (b, t): mel and gmel move as 16-byte vectors when FP is a multiple of 4 and both are 16-byte aligned.
template <int CH>
MSMC_DEV float sp_image1_grad(float m, float gi) {
    if (CH == 0) return gi;
    const float lg = (20.f * log10f(m) - 20.f + 100.f) / 100.f;
    return (lg > 0.f && lg < 1.f) ? gi * (0.2f / (2.302585092994046f * m)) : 0.f;
}
template <typename O, int CH>
MSMC_DEV void mrd_image1_bwd_body(const float* __restrict__ mel, const O* __restrict__ gimg,
                                                            float* __restrict__ gmel, int T, int F, int FP, long total, int bid, int nb) {
    const bool vec = (FP % 4) == 0 && ((size_t)mel % 16) == 0 && ((size_t)gmel % 16) == 0;
    const long nrun = (total + 3) / 4;
    for (long q = (long)bid * 256 + threadIdx.x; q < nrun; q += (long)nb * 256) {
        const long e0 = q * 4;
        if (vec) {                                      // (total = B T FP is a multiple of 4 and the run stays in one row)
            const int f0 = (int)(e0 % FP);
            const long r = e0 / FP;                     // b*T + t
            const int t = (int)(r % T);
            const long b = r / T;
            const f32x4 m4 = *(const f32x4*)(mel + e0);
            float gi[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) gi[u] = f0 + u < F ? sp_load1(gimg + ((b * F + f0 + u) * (long)T) + t) : 0.f;
            f32x4 g4;
#pragma unroll
            for (int u = 0; u < 4; ++u) g4[u] = f0 + u < F ? sp_image1_grad<CH>(m4[u], gi[u]) : 0.f;
            *(f32x4*)(gmel + e0) = g4;
            continue;
        }
        for (long e = e0; e < e0 + 4 && e < total; ++e) {
            const int f = (int)(e % FP);
            const long r = e / FP;
            const int t = (int)(r % T);
            const long b = r / T;
            gmel[e] = f < F ? sp_image1_grad<CH>(mel[e], sp_load1(gimg + ((b * F + f) * (long)T) + t)) : 0.f;
        }
    }
}
template <typename O, int CH>
__global__ __launch_bounds__(256) void mrd_image1_bwd_kernel(const float* __restrict__ mel, const O* __restrict__ gimg,
                                                            float* __restrict__ gmel, int T, int F, int FP, long total) {
    mrd_image1_bwd_body<O, CH>(mel, gimg, gmel, T, F, FP, total, (int)blockIdx.x, (int)gridDim.x);
}
// (dtype, channel) -> instantiation of a single-channel image body or kernel
#define SP_IMAGE1(dtype, channel, GO)                             \
    do {                                                          \
        if ((dtype) == 0) {                                       \
            if ((channel) == 0) GO(float, 0);                     \
            else GO(float, 1);                                    \
        } else {                                                  \
            if ((channel) == 0) GO(unsigned short, 0);            \
            else GO(unsigned short, 1);                           \
        }                                                         \
    } while (0)

MSMC_DEV void log_clamp_fwd_body(const float* __restrict__ x, float* __restrict__ y, long n,
                                                           float lo, int bid, int nb) {
    for (long e = (long)bid * 256 + threadIdx.x; e < n; e += (long)nb * 256) {
        const float v = x[e];
        y[e] = logf(v < lo ? lo : v);
    }
}
__global__ __launch_bounds__(256) void log_clamp_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long n,
                                                           float lo) {
    log_clamp_fwd_body(x, y, n, lo, (int)blockIdx.x, (int)gridDim.x);
}
MSMC_DEV void log_clamp_bwd_body(const float* __restrict__ x, const float* __restrict__ g,
                                                           float* __restrict__ gx, long n, float lo, int bid, int nb) {
    for (long e = (long)bid * 256 + threadIdx.x; e < n; e += (long)nb * 256) {
        const float v = x[e];
        gx[e] = v > lo ? g[e] / v : 0.f;
    }
}
__global__ __launch_bounds__(256) void log_clamp_bwd_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                           float* __restrict__ gx, long n, float lo) {
    log_clamp_bwd_body(x, g, gx, n, lo, (int)blockIdx.x, (int)gridDim.x);
}

// Several of the element-wise stages above in ONE launch (msmc_spectral_multi): the five resolution discriminators' front-ends
// are five identical chains frames -> DFT -> magnitude -> filter bank -> image over different hop lengths, each stage a launch of
// 5-10 us for a microsecond of work, and a chain of 25 such launches sat on the step's critical chain forward and again
// backward (profiles/r06_step_timeline_start_of_round.txt).  A block looks its operation up in the argument and runs the stage's
// own body over its share of the operation's elements.
struct SpMultiArgs {
    int n;
    int first[MSMC_SPECTRAL_MULTI_MAX + 1];
    msmc_spectral_op op[MSMC_SPECTRAL_MULTI_MAX];
};
__global__ __launch_bounds__(256) void spectral_multi_kernel(SpMultiArgs a) {
    int k = 0;
    while (k + 1 < a.n && (int)blockIdx.x >= a.first[k + 1]) ++k;
    const msmc_spectral_op& o = a.op[k];
    const int bid = (int)blockIdx.x - a.first[k], nb = a.first[k + 1] - a.first[k];
    switch (o.kind) {
        case 0: stft_frames_fwd_body((const float*)o.a, (float*)o.out, o.L, o.T, o.n_fft, o.NP, o.hop, o.pad, (long)o.B * o.T * o.NP, bid, nb); break;
        case 1: stft_frames_bwd_body((const float*)o.a, (float*)o.out, o.L, o.T, o.n_fft, o.NP, o.hop, o.pad, (long)o.B * o.L, bid, nb); break;
        case 2: spec_mag_fwd_body((const float*)o.a, (float*)o.out, o.F, o.CP, o.FP, o.lo, o.clamp_mode, o.R * o.FP, bid, nb); break;
        case 3: spec_mag_bwd_body((const float*)o.a, (const float*)o.b, (const float*)o.c, (float*)o.out, o.F, o.CP, o.FP, o.lo, o.clamp_mode, o.R * o.CP, bid, nb); break;
        case 4:
            if (o.dtype == 0) mrd_image_fwd_body<float>((const float*)o.a, (float*)o.out, o.T, o.F, o.FP, (long)o.B * o.F * o.T, bid, nb);
            else mrd_image_fwd_body<unsigned short>((const float*)o.a, (unsigned short*)o.out, o.T, o.F, o.FP, (long)o.B * o.F * o.T, bid, nb);
            break;
        case 8: {
#define SP_GO(O_, CH_) mrd_image1_fwd_body<O_, CH_>((const float*)o.a, (O_*)o.out, o.T, o.F, o.FP, (long)o.B * o.F * o.T, bid, nb)
            SP_IMAGE1(o.dtype, o.channel, SP_GO);
#undef SP_GO
            break;
        }
        case 9: {
#define SP_GO(O_, CH_) mrd_image1_bwd_body<O_, CH_>((const float*)o.a, (const O_*)o.b, (float*)o.out, o.T, o.F, o.FP, (long)o.B * o.T * o.FP, bid, nb)
            SP_IMAGE1(o.dtype, o.channel, SP_GO);
#undef SP_GO
            break;
        }
        case 6: log_clamp_fwd_body((const float*)o.a, (float*)o.out, o.R, o.lo, bid, nb); break;
        case 7: log_clamp_bwd_body((const float*)o.a, (const float*)o.b, (float*)o.out, o.R, o.lo, bid, nb); break;
        default:
            if (o.dtype == 0) mrd_image_bwd_body<float>((const float*)o.a, (const float*)o.b, (float*)o.out, o.T, o.F, o.FP, (long)o.B * o.T * o.FP, bid, nb);
            else mrd_image_bwd_body<unsigned short>((const float*)o.a, (const unsigned short*)o.b, (float*)o.out, o.T, o.F, o.FP, (long)o.B * o.T * o.FP, bid, nb);
            break;
    }
}

static inline dim3 sp_grid(long total) {
    long b = (total + 1023) / 1024;
    if (b > 2048) b = 2048;
    if (b < 1) b = 1;
    return dim3((unsigned)b);
}

// ---- waveform fan-out of the discriminator (reference hifigan/discriminator.py:102-116,135-145,180-190) ------------------
// One generated waveform feeds five resolution sub-discriminators (fp32 spectral front-ends) and five period sub-discriminators
// (a cast to the stack's dtype, a reflection pad to a multiple of the period for two of them, a fold).  As stock operators that
// is a cast + two pads forward and, backward, two pad gradients, a cast gradient and ~20 accumulations of [B][L] gradients by
// the autograd engine.  Forward here: every period's padded copy in ONE launch; backward: the sum of all consumers' gradients
// (fp32 front-end gradients + padded period gradients folded at the reflected tail) in ONE launch.
#define WF_MAX 8
struct WaveFanArgs {
    int n16, n32;                       // period copies / fp32 gradient tensors
    int Lp[WF_MAX];                     // padded length of copy k
    void* p16[WF_MAX];                  // copies [B][Lp[k]] (forward: written; backward: their gradients, NULL = none)
    const float* p32[WF_MAX];           // backward only: fp32 gradients [B][L] (NULL = none)
};
template <typename T>
__global__ __launch_bounds__(256) void wave_fan_fwd_kernel(const float* __restrict__ y, WaveFanArgs a, int L, int Lmax,
                                                          long total) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int t = (int)(e % Lmax);
        const long b = e / Lmax;
        const float v = y[b * L + sp_reflect(t, L)];
#pragma unroll
        for (int k = 0; k < WF_MAX; ++k)
            if (k < a.n16 && t < a.Lp[k]) {
                if (sizeof(T) == 4) ((float*)a.p16[k])[b * a.Lp[k] + t] = v;
                else ((unsigned short*)a.p16[k])[b * a.Lp[k] + t] = f32_to_bf16_bits(v);
            }
    }
}
template <typename T>
__global__ __launch_bounds__(256) void wave_fan_bwd_kernel(WaveFanArgs a, float* __restrict__ gy, int L, long total) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int l = (int)(e % L);
        const long b = e / L;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < WF_MAX; ++k)
            if (k < a.n32 && a.p32[k]) s = s + a.p32[k][e];
        const int tr = 2 * (L - 1) - l;                  // padded position that reflects onto l (tail only: tr >= L)
#pragma unroll
        for (int k = 0; k < WF_MAX; ++k)
            if (k < a.n16 && a.p16[k]) {
                const long base = b * a.Lp[k];
                if (sizeof(T) == 4) {
                    const float* g = (const float*)a.p16[k];
                    s = s + g[base + l];
                    if (tr >= L && tr < a.Lp[k]) s = s + g[base + tr];
                } else {
                    const unsigned short* g = (const unsigned short*)a.p16[k];
                    s = s + bf16_bits_to_f32(g[base + l]);
                    if (tr >= L && tr < a.Lp[k]) s = s + bf16_bits_to_f32(g[base + tr]);
                }
            }
        gy[e] = s;
    }
}

// The vocoder windows of a captured step (reference msmctts_trainer.py:211-219 random_select, as device arithmetic): frame indices
// start_b + i and the waveform window wav[b][start_b * hop + j] of every utterance in ONE launch -- the operator chain (two
// aranges, a multiply, two broadcast adds, a gather) was six launches at the head of the step's critical chain.
__global__ __launch_bounds__(256) void window_gather_kernel(const long* __restrict__ starts, const float* __restrict__ wav,
                                                           long* __restrict__ frames, float* __restrict__ target, int nframes,
                                                           int hop, long L, long total) {
    const long per = (long)nframes * hop;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long b = e / per, j = e - b * per;
        const long s0 = starts[b];
        target[e] = wav[b * L + s0 * hop + j];
        if (j < nframes) frames[b * nframes + j] = s0 + j;
    }
}

// Operands of the framing pair (and of kinds 0 / 1 of msmc_spectral_multi): sp_reflect folds an index once, so the last padded
// position a frame reads, (T-1)*hop + n_fft - 1 - pad, must not pass the single right reflection's end 2L - 2 (L > pad keeps the
// left one inside).
static inline bool sp_frames_ok(int B, int L, int T, int n_fft, int NP, int hop, int pad) {
    if (B <= 0 || L <= pad || T <= 0 || NP < n_fft || hop <= 0 || pad < 0) return false;
    return (long)(T - 1) * hop + n_fft - 1 - pad <= 2 * (long)L - 2;
}

extern "C" {

int msmc_stft_frames_fwd(const float* x, float* frames, int B, int L, int T, int n_fft, int NP, int hop, int pad,
                         msmc_stream stream) {
    if (!x || !frames || !sp_frames_ok(B, L, T, n_fft, NP, hop, pad)) return MSMC_E_SHAPE;
    const long total = (long)B * T * NP;
    MSMC_LAUNCH(stft_frames_fwd_kernel, sp_grid(total), dim3(256), 0, (msmc_stream_t)stream, x, frames, L, T, n_fft, NP,
                hop, pad, total);
    return msmc_check_launch();
}
int msmc_stft_frames_bwd(const float* gframes, float* gx, int B, int L, int T, int n_fft, int NP, int hop, int pad,
                         msmc_stream stream) {
    if (!gframes || !gx || !sp_frames_ok(B, L, T, n_fft, NP, hop, pad)) return MSMC_E_SHAPE;
    const long total = (long)B * L;
    MSMC_LAUNCH(stft_frames_bwd_kernel, sp_grid(total), dim3(256), 0, (msmc_stream_t)stream, gframes, gx, L, T, n_fft, NP,
                hop, pad, total);
    return msmc_check_launch();
}
int msmc_spec_mag_fwd(const float* spec, float* mag, long R, int F, int CP, int FP, float lo, int clamp_mode,
                      msmc_stream stream) {
    if (!spec || !mag || R <= 0 || F <= 0 || CP < 2 * F || FP < F) return MSMC_E_SHAPE;
    const long total = R * FP;
    MSMC_LAUNCH(spec_mag_fwd_kernel, sp_grid(total), dim3(256), 0, (msmc_stream_t)stream, spec, mag, F, CP, FP, lo,
                clamp_mode, total);
    return msmc_check_launch();
}
int msmc_spec_mag_bwd(const float* spec, const float* mag, const float* gmag, float* gspec, long R, int F, int CP,
                      int FP, float lo, int clamp_mode, msmc_stream stream) {
    if (!spec || !mag || !gmag || !gspec || R <= 0 || F <= 0 || CP < 2 * F || FP < F) return MSMC_E_SHAPE;
    const long total = R * CP;
    MSMC_LAUNCH(spec_mag_bwd_kernel, sp_grid(total), dim3(256), 0, (msmc_stream_t)stream, spec, mag, gmag, gspec, F, CP,
                FP, lo, clamp_mode, total);
    return msmc_check_launch();
}
int msmc_mrd_image_fwd_dt(const float* mel, void* img, int B, int T, int F, int FP, int dtype, msmc_stream stream) {
    if (!mel || !img || B <= 0 || T <= 0 || F <= 0 || FP < F || dtype < 0 || dtype > 1) return MSMC_E_SHAPE;
    const long total = (long)B * F * T;
    if (dtype == 0)
        MSMC_LAUNCH(mrd_image_fwd_kernel<float>, sp_grid(total), dim3(256), 0, (msmc_stream_t)stream, mel, (float*)img, T, F, FP,
                    total);
    else
        MSMC_LAUNCH(mrd_image_fwd_kernel<unsigned short>, sp_grid(total), dim3(256), 0, (msmc_stream_t)stream, mel,
                    (unsigned short*)img, T, F, FP, total);
    return msmc_check_launch();
}
int msmc_mrd_image_bwd_dt(const float* mel, const void* gimg, float* gmel, int B, int T, int F, int FP, int dtype,
                          msmc_stream stream) {
    if (!mel || !gimg || !gmel || B <= 0 || T <= 0 || F <= 0 || FP < F || dtype < 0 || dtype > 1) return MSMC_E_SHAPE;
    const long total = (long)B * T * FP;
    if (dtype == 0)
        MSMC_LAUNCH(mrd_image_bwd_kernel<float>, sp_grid(total), dim3(256), 0, (msmc_stream_t)stream, mel, (const float*)gimg,
                    gmel, T, F, FP, total);
    else
        MSMC_LAUNCH(mrd_image_bwd_kernel<unsigned short>, sp_grid(total), dim3(256), 0, (msmc_stream_t)stream, mel,
                    (const unsigned short*)gimg, gmel, T, F, FP, total);
    return msmc_check_launch();
}
int msmc_mrd_image1_fwd_dt(const float* mel, void* img, int B, int T, int F, int FP, int channel, int dtype, msmc_stream stream) {
    if (!mel || !img || B <= 0 || T <= 0 || F <= 0 || FP < F || channel < 0 || channel > 1 || dtype < 0 || dtype > 1) return MSMC_E_SHAPE;
    const long total = (long)B * F * T;
#define SP_GO(O_, CH_)                                                                                                          \
    MSMC_LAUNCH((mrd_image1_fwd_kernel<O_, CH_>), sp_grid((total + 3) / 4), dim3(256), 0, (msmc_stream_t)stream, mel, (O_*)img, T, F, \
                FP, total)
    SP_IMAGE1(dtype, channel, SP_GO);
#undef SP_GO
    return msmc_check_launch();
}
int msmc_mrd_image1_bwd_dt(const float* mel, const void* gimg, float* gmel, int B, int T, int F, int FP, int channel, int dtype,
                           msmc_stream stream) {
    if (!mel || !gimg || !gmel || B <= 0 || T <= 0 || F <= 0 || FP < F || channel < 0 || channel > 1 || dtype < 0 || dtype > 1)
        return MSMC_E_SHAPE;
    const long total = (long)B * T * FP;
#define SP_GO(O_, CH_)                                                                                                          \
    MSMC_LAUNCH((mrd_image1_bwd_kernel<O_, CH_>), sp_grid((total + 3) / 4), dim3(256), 0, (msmc_stream_t)stream, mel,            \
                (const O_*)gimg, gmel, T, F, FP, total)
    SP_IMAGE1(dtype, channel, SP_GO);
#undef SP_GO
    return msmc_check_launch();
}
int msmc_mrd_image_fwd(const float* mel, float* img, int B, int T, int F, int FP, msmc_stream stream) {
    return msmc_mrd_image_fwd_dt(mel, img, B, T, F, FP, 0, stream);
}
int msmc_mrd_image_bwd(const float* mel, const float* gimg, float* gmel, int B, int T, int F, int FP,
                       msmc_stream stream) {
    return msmc_mrd_image_bwd_dt(mel, gimg, gmel, B, T, F, FP, 0, stream);
}
int msmc_log_clamp_fwd(const float* x, float* y, long n, float lo, msmc_stream stream) {
    if (!x || !y || n <= 0) return MSMC_E_SHAPE;
    MSMC_LAUNCH(log_clamp_fwd_kernel, sp_grid(n), dim3(256), 0, (msmc_stream_t)stream, x, y, n, lo);
    return msmc_check_launch();
}
int msmc_log_clamp_bwd(const float* x, const float* g, float* gx, long n, float lo, msmc_stream stream) {
    if (!x || !g || !gx || n <= 0) return MSMC_E_SHAPE;
    MSMC_LAUNCH(log_clamp_bwd_kernel, sp_grid(n), dim3(256), 0, (msmc_stream_t)stream, x, g, gx, n, lo);
    return msmc_check_launch();
}


int msmc_wave_fan_fwd(const float* y, void* const* copies, const int* padded_len, int n, int B, int L, int dtype,
                      msmc_stream stream) {
    if (!y || !copies || !padded_len || n <= 0 || n > WF_MAX || B <= 0 || L <= 1 || dtype < 0 || dtype > 1) return MSMC_E_SHAPE;
    WaveFanArgs a;
    a.n16 = n;
    a.n32 = 0;
    int Lmax = 0;
    for (int k = 0; k < n; ++k) {
        if (!copies[k] || padded_len[k] < L || padded_len[k] > 2 * L - 1) return MSMC_E_SHAPE;   // (one reflection at most)
        a.p16[k] = copies[k];
        a.Lp[k] = padded_len[k];
        if (padded_len[k] > Lmax) Lmax = padded_len[k];
    }
    const long total = (long)B * Lmax;
    if (dtype == 0) MSMC_LAUNCH(wave_fan_fwd_kernel<float>, sp_grid(total), dim3(256), 0, (msmc_stream_t)stream, y, a, L, Lmax, total);
    else MSMC_LAUNCH(wave_fan_fwd_kernel<unsigned short>, sp_grid(total), dim3(256), 0, (msmc_stream_t)stream, y, a, L, Lmax, total);
    return msmc_check_launch();
}
int msmc_wave_fan_bwd(const float* const* g32, int n32, const void* const* gcopies, const int* padded_len, int n, float* gy,
                      int B, int L, int dtype, msmc_stream stream) {
    if (!gy || n < 0 || n > WF_MAX || n32 < 0 || n32 > WF_MAX || B <= 0 || L <= 1 || dtype < 0 || dtype > 1) return MSMC_E_SHAPE;
    if ((n && (!gcopies || !padded_len)) || (n32 && !g32)) return MSMC_E_SHAPE;
    WaveFanArgs a;
    a.n16 = n;
    a.n32 = n32;
    for (int k = 0; k < n; ++k) {
        if (padded_len[k] < L || padded_len[k] > 2 * L - 1) return MSMC_E_SHAPE;
        a.p16[k] = (void*)gcopies[k];
        a.Lp[k] = padded_len[k];
    }
    for (int k = 0; k < n32; ++k) a.p32[k] = g32[k];
    const long total = (long)B * L;
    if (dtype == 0) MSMC_LAUNCH(wave_fan_bwd_kernel<float>, sp_grid(total), dim3(256), 0, (msmc_stream_t)stream, a, gy, L, total);
    else MSMC_LAUNCH(wave_fan_bwd_kernel<unsigned short>, sp_grid(total), dim3(256), 0, (msmc_stream_t)stream, a, gy, L, total);
    return msmc_check_launch();
}
int msmc_window_gather(const long* starts, const float* wav, long* frames, float* target, int B, int nframes, int hop, long L,
                       msmc_stream stream) {
    if (!starts || !wav || !frames || !target || B <= 0 || nframes <= 0 || hop <= 0 || L < (long)nframes * hop) return MSMC_E_SHAPE;
    const long total = (long)B * nframes * hop;
    MSMC_LAUNCH(window_gather_kernel, sp_grid(total), dim3(256), 0, (msmc_stream_t)stream, starts, wav, frames, target, nframes, hop, L,
                total);
    return msmc_check_launch();
}
int msmc_spectral_multi(const msmc_spectral_op* ops, int n, msmc_stream stream) {
    if (!ops || n <= 0 || n > MSMC_SPECTRAL_MULTI_MAX) return MSMC_E_SHAPE;
    SpMultiArgs a;
    a.n = n;
    int blocks = 0;
    for (int k = 0; k < n; ++k) {
        const msmc_spectral_op& o = ops[k];
        long total;
        if (!o.a || !o.out) return MSMC_E_SHAPE;
        switch (o.kind) {
            case 0: case 1:
                if (!sp_frames_ok(o.B, o.L, o.T, o.n_fft, o.NP, o.hop, o.pad)) return MSMC_E_SHAPE;
                total = o.kind == 0 ? (long)o.B * o.T * o.NP : (long)o.B * o.L;
                break;
            case 2: case 3:
                if (o.R <= 0 || o.F <= 0 || o.CP < 2 * o.F || o.FP < o.F || (o.kind == 3 && (!o.b || !o.c))) return MSMC_E_SHAPE;
                total = o.kind == 2 ? o.R * o.FP : o.R * o.CP;
                break;
            case 4: case 5:
                if (o.B <= 0 || o.T <= 0 || o.F <= 0 || o.FP < o.F || o.dtype < 0 || o.dtype > 1 || (o.kind == 5 && !o.b)) return MSMC_E_SHAPE;
                total = o.kind == 4 ? (long)o.B * o.F * o.T : (long)o.B * o.T * o.FP;
                break;
            case 8: case 9:
                if (o.B <= 0 || o.T <= 0 || o.F <= 0 || o.FP < o.F || o.dtype < 0 || o.dtype > 1 || o.channel < 0 || o.channel > 1 ||
                    (o.kind == 9 && !o.b)) return MSMC_E_SHAPE;
                total = ((o.kind == 8 ? (long)o.B * o.F * o.T : (long)o.B * o.T * o.FP) + 3) / 4;      // (a lane owns four elements)
                break;
            case 6: case 7:
                if (o.R <= 0 || (o.kind == 7 && !o.b)) return MSMC_E_SHAPE;
                total = o.R;
                break;
            default: return MSMC_E_SHAPE;
        }
        a.first[k] = blocks;
        a.op[k] = o;
        blocks += (int)sp_grid(total).x;
    }
    a.first[n] = blocks;
    MSMC_LAUNCH(spectral_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, (msmc_stream_t)stream, a);
    return msmc_check_launch();
}
}  // extern "C"
