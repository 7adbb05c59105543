// griffin_lim.hip -- spectrogram and mel back to waveform, for gfx950: the linear spectrogram and the Griffin-Lim inverses that the
// reference computes per file on the CPU (examples/csmsc/scripts/audio/audio.py: inv_preemphasis :27-28, spectrogram :31-34,
// fast_inv_spectrogram / inv_mel_spectrogram / inv_spectrogram :37-56, _stft / _istft :71-78, _fast_griffin_lim / _griffin_lim
// :176-204 -- 60 iterations of librosa.stft + librosa.istft).  Host side: msmctts_amd/hip/griffin_lim.py (GriffinLim builds the
// constant matrices and runs the loop: two launches per iteration); tools: tools/invert_features.py, tools/extract_features.py.
//
// ---- msmc_stft: wav [B][Lmax] fp32, length [B] (device) -> one of three outputs on the frame grid of features.hip ----------------
//   T_b = 1 + L_b / hop frames, each utterance reflect-padded by n_fft / 2 at its own length, optional pre-emphasis (0: none),
//   re / im[t][f] = sum_n frame[t][n] basis[n][f] with the windowed basis of features.py (windowed_dft_basis).
// The work mapping, the tiling (GL_FT = 32 frames per workgroup, GL_FQ = 128 frequencies per tile, 32 per wave, GL_KS = 16 taps per
// basis slice, double-buffered in LDS, one barrier per slice) and the v_mfma_f32_32x32x2_f32 main loop are those of
// mel_features_kernel (features.hip), restated here so that the object code of that kernel stays as it is; re and im therefore
// carry its tap order.  Lane (i, h) = (lane & 31, lane >> 5) of wave w ends a frequency tile with re / im of frequency
// f = 128 tile + 32 w + i for the 16 frames (r & 3) + 8 (r >> 2) + 4 h, and writes them itself (128 B per wave and frame row):
//   mode 0 (complex): out [B][Tmax][2][F] fp32 -- per frame the F real parts, then the F imaginary parts (planar per frame: a
//                     frame's row of 2 F floats is the K operand of msmc_istft as it stands).
//   mode 1 (project): one Griffin-Lim projection onto the magnitudes mag [B][Tmax][F]: t1 = mag z / |z| in the layout of mode 0;
//                     z == 0 exactly gives (mag, 0), as numpy's angle(0) = 0.  |z| is formed without overflow or underflow:
//                     m = max(|re|, |im|), u = re / m, v = im / m, q = sqrt(u u + v v), t1 = (mag (u / q), mag (v / q)) -- IEEE
//                     divisions and square root: 3 units of 2^-24 relative to mag per component by the first-order count (the
//                     tests assert 4).  With prev (layout of mode 0, holding t0): out = t1 + alpha (t1 - t0) (subtract, multiply,
//                     add: three roundings) and prev = t1, every element read and written by the same work-item
//                     (_fast_griffin_lim).
//   mode 2 (db):      out [B][Tmax][F] = clip(normalise(20 log10(max(1e-5, sqrt(re^2 + im^2))) - ref_level_db)), the epilogue of
//                     features.hip per frequency; with pre-emphasis this is audio.spectrogram.
//   Rows t >= T_b of out are +0 in every mode (prev is not touched there).
// SUMMATION ORDER: taps in ascending order from +0, one fmaf per tap (the zero rows that pad win to whole slices come last).  No
// atomics; frame tiles start at multiples of 32 frames of the utterance, so neither the batch nor Lmax changes a bit.
//
// ---- msmc_istft: spec [B][Tmax][2][F] fp32, frames [B] (device) -> y [B][hop (Tmax - 1)] fp32: librosa.istft with its defaults ----
//   frame t = irfft(spec[t], n_fft) times the periodic Hann window of win samples centred in n_fft; overlap-add at t hop; the sum is
//   divided by the sum of the squared windows where that exceeds the smallest normal fp32 (FLT_MIN), else left as it is; n_fft / 2
//   trimmed at both ends: hop (T_b - 1) samples, +0 behind them.  Only the win taps under the window are computed:
//     frame[t][n] = sum_k spec[t][k] ibasis[k][n],  k < F: c_f w[n] cos(2 pi f (n + off) / n_fft) / n_fft against re[f = k],
//                                                    k >= F: -c_f w[n] sin(...) / n_fft against im[f = k - F],
//   c_f = 1 for DC and Nyquist (whose imaginary rows are zero), 2 otherwise; off = (n_fft - win) / 2.
// In the window's own coordinate u = (position in the untrimmed sum) - off, frame t covers u in [t hop, t hop + win) with tap
// n = u - t hop, and output sample j is u = j + c, c = n_fft / 2 - off.  So the frames that reach a stretch of u lie on ONE side of
// it: with H = ceil(win / hop) - 1, the halo, a workgroup of four waves owns u in [q PT hop, (q + 1) PT hop), PT = 32 - H frame
// positions of one utterance (grid: tiles x utterances), and computes the 32 frames t = q PT - H .. q PT + PT - 1 that exist (rows
// with t < 0 or t >= T_b are zero rows): an fp32 MFMA GEMM [32 frames][K = 2 F] x [K][win], the taps in tiles of 128 (32 per
// wave), K in slices of 16: a slice of the spectrum rows ([32][16], pitch 17) and of the basis ([16][128], contiguous in the host's
// layout [tile][KP][128]) travel L2 -> registers (issued ahead of the slice's MFMAs) -> the other of two LDS buffers (behind
// them), one barrier per slice.  The 32 x win windowed frames stay in LDS; then work-item e gathers sample u = q PT hop + e (+ 256):
//   acc = sum over t = max(0, ceil((u - win + 1) / hop)) .. min(T_b - 1, u / hop) ASCENDING of frame[t][u - t hop], from +0,
//   env = the sum of wsq[u - t hop] in the same order from +0 (wsq: the squared window, float64 rounded to fp32 once),
//   y[j] = env > FLT_MIN ? acc / env : acc.
// The H frames of the halo are computed again by the neighbouring workgroup; no atomics, no second pass.  hop >= win: H = 0, the
// samples between two windows keep acc = +0.
// SUMMATION ORDER of K: k ascending from +0, one fmaf each -- the real parts f = 0 .. F - 1, then the imaginary parts f = 0 ..
// F - 1 (the zero rows that pad 2 F to whole slices come last).  A sample depends on its utterance's frames and count only.
//
// ---- msmc_deemphasis: y[n] = x[n] + a y[n - 1] (inv_preemphasis) per utterance, n < length[b]; x == y allowed -------------------
// One workgroup per utterance walks chunks of 256 samples with a carry (the last y of the chunk before; +0 at the start), as
// collapse_units carries its run count.  Inside a chunk, work-item i holds v = x[i] (work-item 0: x[0] + a carry) and eight
// steps d = 1, 2, 4 .. 128 do v[i] = v[i] + p_d v[i - d] for i >= d, with p_1 = a and p_2d = p_d p_d in fp32 (multiply, then add:
// the build does not contract).  Samples at or behind the length are neither read nor written.
//
// Who guarantees what.  THE KERNELS CHECK: length[b] / frames[b] are clamped to [0, Lmax] / [0, Tmax]; an utterance with length
// <= n_fft / 2 gives zero rows; every sample index is tested against [0, L_b) after the reflection and every frame row against
// [0, T_b), so no address outside a row is formed.  THE LAUNCHERS CHECK: the accepted shapes (msmc_hip.h, A4) and that the LDS
// fits; MSMC_E_SHAPE launches nothing.  THE CALLER GUARANTEES: the buffers' shapes, contiguous, 16-byte aligned.
#include <float.h>
#include <msmc_rt.hpp>
#include <msmc_hip.h>

#define GL_FT 32                         // frames per workgroup (both transforms)
#define GL_FQ 128                        // frequencies (stft) / taps (istft) per tile, 32 per wave
#define GL_KS 16                         // taps (stft) / spectrum entries (istft) per slice
#define GL_WG 256
#define GL_SLICE (GL_KS * 2 * GL_FQ)     // stft: [KS][cos FQ | -sin FQ]
#define GL_ISLICE (GL_KS * GL_FQ)        // istft: [KS][FQ]
#define GL_AP (GL_KS + 1)                // istft: pitch of a spectrum slice row
#define GL_LDS_MAX (160 * 1024)
#define GL_CHUNK 256                     // de-emphasis: samples per step of the carry

struct StftArgs {
    const float* wav;
    const int* length;
    const float* basis;
    const float* mag;
    float* out;
    float* prev;
    int mode, Lmax, Tmax, n_fft, win, hop, F;
    int WP, nft;                         // padded taps, frequency tiles
    int P, span_real, span_floats;       // frame pitch in the span, its samples, its floats in LDS (zeros behind the samples)
    float pre, alpha, ref_db, min_db, max_abs;
    int symmetric;
};

// audio.py:114-129 on one amplitude (feat_normalise of features.hip)
MSMC_DEV float gl_normalise(float m, const StftArgs& a) {
    const float S = 20.f * log10f(fmaxf(1e-5f, m)) - a.ref_db;
    const float u = (S - a.min_db) / (-a.min_db);
    if (a.symmetric) return fminf(fmaxf((2.f * a.max_abs) * u - a.max_abs, -a.max_abs), a.max_abs);
    return fminf(fmaxf(a.max_abs * u, 0.f), a.max_abs);
}

__global__ __launch_bounds__(GL_WG) void stft_kernel(StftArgs a) {
    MSMC_DYN_LDS(smem);
    float* span = (float*)smem;                          // [span_floats]
    float* bs = span + a.span_floats;                    // [2][KS][cos FQ | -sin FQ]
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int i = lane & 31, h = lane >> 5;
    const int b = blockIdx.y, t0 = blockIdx.x * GL_FT;
    const int half = a.n_fft >> 1, F = a.F;
    int L = a.length[b];
    L = L < 0 ? 0 : (L > a.Lmax ? a.Lmax : L);
    int Tb = L > half ? 1 + L / a.hop : 0;
    if (Tb > a.Tmax) Tb = a.Tmax;
    const int width = a.mode == 2 ? F : 2 * F;           // floats per frame row of out
    float* out = a.out + (size_t)b * a.Tmax * width;

    if (t0 >= Tb) {                                      // (the same in every work-item) nothing but zero rows in this tile
        const int rows = a.Tmax - t0 < GL_FT ? a.Tmax - t0 : GL_FT;
        for (int e = tid; e < rows * width; e += GL_WG) out[(size_t)t0 * width + e] = 0.f;
        return;
    }

    // the tile's samples: reflect the index at 0 and at L, then pre-emphasise at that index
    {
        const float* y = a.wav + (size_t)b * a.Lmax;
        const long first = (long)t0 * a.hop + ((a.n_fft - a.win) >> 1) - half;
        for (int e = tid; e < a.span_floats; e += GL_WG) {
            float v = 0.f;
            if (e < a.span_real) {
                const long pos = a.hop < a.win ? (long)e : (long)(e / a.win) * a.hop + e % a.win;
                long j = first + pos;
                if (j < 0) j = -j;
                if (j >= L) j = 2 * ((long)L - 1) - j;
                if (j >= 0 && j < L) {
                    v = y[j];
                    if (j > 0) v = v - a.pre * y[j - 1];
                }
            }
            span[e] = v;
        }
    }

    const int nks = a.WP / GL_KS, total = a.nft * nks;
    f32x4 st[4];                                         // a basis slice in flight: 1024 16-byte pieces over 256 work-items
    auto load = [&](int q) {
        const float* src = a.basis + (size_t)q * GL_SLICE;
#pragma unroll
        for (int n = 0; n < 4; ++n) st[n] = *(const f32x4*)(src + 4 * (n * GL_WG + tid));
    };
    auto store = [&](int buf) {
        float* dst = bs + buf * GL_SLICE;
#pragma unroll
        for (int n = 0; n < 4; ++n) *(f32x4*)(dst + 4 * (n * GL_WG + tid)) = st[n];
    };
    load(0);
    store(0);
    __syncthreads();

    f32x16 re, im;
    int buf = 0;
    for (int q = 0; q < total; ++q) {
        const int ft = q / nks, ks = q - ft * nks;
        const bool more = q + 1 < total;
        if (more) load(q + 1);
        if (ks == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) re[r] = im[r] = 0.f;
        }
        const float* ap = span + i * a.P + ks * GL_KS + h;
        const float* bp = bs + buf * GL_SLICE + h * (2 * GL_FQ) + w * 32 + i;
#pragma unroll
        for (int s = 0; s < GL_KS / 2; ++s) {            // taps 2 s + h
            const float av = ap[2 * s];
            const float cv = bp[2 * s * (2 * GL_FQ)], sv = bp[2 * s * (2 * GL_FQ) + GL_FQ];
            re = mfma_f32_32x32x2(av, cv, re);
            im = mfma_f32_32x32x2(av, sv, im);
        }
        if (more) store(buf ^ 1);

        const int f = ft * GL_FQ + w * 32 + i;
        if (ks == nks - 1 && f < F) {                    // the tile's spectrum is complete: this lane's 16 frames of frequency f
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int t = t0 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (t >= a.Tmax) continue;
                const size_t row = (size_t)t * width;
                const float zr = re[r], zi = im[r];
                if (a.mode == 2) {
                    const float rr = zr * zr, ii = zi * zi;
                    out[row + f] = t < Tb ? gl_normalise(sqrtf(rr + ii), a) : 0.f;
                } else if (t >= Tb) {
                    out[row + f] = 0.f;
                    out[row + F + f] = 0.f;
                } else if (a.mode == 0) {
                    out[row + f] = zr;
                    out[row + F + f] = zi;
                } else {
                    const float S = a.mag[((size_t)b * a.Tmax + t) * F + f];
                    float pr = S, pi = 0.f;
                    if (zr != 0.f || zi != 0.f) {
                        const float m = fmaxf(fabsf(zr), fabsf(zi));
                        const float u = zr / m, v = zi / m;
                        const float uu = u * u, vv = v * v;
                        const float qn = sqrtf(uu + vv);
                        pr = S * (u / qn);
                        pi = S * (v / qn);
                    }
                    if (a.prev) {
                        float* pv = a.prev + (size_t)b * a.Tmax * width + row;
                        const float dr = pr - pv[f], di = pi - pv[F + f];
                        const float er = a.alpha * dr, ei = a.alpha * di;
                        out[row + f] = pr + er;
                        out[row + F + f] = pi + ei;
                        pv[f] = pr;
                        pv[F + f] = pi;
                    } else {
                        out[row + f] = pr;
                        out[row + F + f] = pi;
                    }
                }
            }
        }
        __syncthreads();             // slice q + 1 is complete, and nobody reads slice q any more
        buf ^= 1;
    }
}

struct IstftArgs {
    const float* spec;
    const int* frames;
    const float* ibasis;
    const float* wsq;
    float* y;
    int Tmax, n_fft, win, hop, F;
    int K, nks, ntt;                     // 2 F, slices of K, tap tiles
    int H, PT, c, Lout;                  // halo, frame positions per workgroup, n_fft / 2 - off, hop (Tmax - 1)
};

__global__ __launch_bounds__(GL_WG) void istft_kernel(IstftArgs a) {
    MSMC_DYN_LDS(smem);
    float* fr = (float*)smem;                            // [FT][win]: the windowed frames of this workgroup
    float* as = fr + GL_FT * a.win;                      // [2][FT][AP]
    float* bs = as + 2 * GL_FT * GL_AP;                  // [2][KS][FQ]
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int i = lane & 31, h = lane >> 5;
    const int b = blockIdx.y, q0 = blockIdx.x;
    int Tb = a.frames[b];
    Tb = Tb < 0 ? 0 : (Tb > a.Tmax ? a.Tmax : Tb);
    const int Lb = Tb > 0 ? a.hop * (Tb - 1) : 0;        // this utterance's samples
    const int tq = q0 * a.PT - a.H;                      // frame of row 0 (may be negative)
    const long u0 = (long)q0 * a.PT * a.hop;             // first owned u
    const int owned = a.PT * a.hop;
    float* y = a.y + (size_t)b * a.Lout;

    // nothing to compute where no owned sample lies inside the utterance: zeros (the same in every work-item)
    if (u0 - a.c >= Lb || tq >= Tb) {
        for (int e = tid; e < owned; e += GL_WG) {
            const long j = u0 + e - a.c;
            if (j >= 0 && j < a.Lout) y[j] = 0.f;
        }
        return;
    }

    const float* spec = a.spec + (size_t)b * a.Tmax * a.K;
    const int arow = tid >> 3, ak = 2 * (tid & 7);       // this work-item's two entries of a spectrum slice
    const int at = tq + arow;
    const bool alive = at >= 0 && at < Tb;
    f32x2 sa;
    f32x4 sb[2];
    auto load = [&](int q) {
        const int tt = q / a.nks, ks = q - tt * a.nks;
        const int k = ks * GL_KS + ak;                   // (K is even: k and k + 1 are inside together)
        sa[0] = sa[1] = 0.f;
        if (alive && k < a.K) sa = *(const f32x2*)(spec + (size_t)at * a.K + k);
        const float* src = a.ibasis + (size_t)q * GL_ISLICE;
#pragma unroll
        for (int n = 0; n < 2; ++n) sb[n] = *(const f32x4*)(src + 4 * (n * GL_WG + tid));
        (void)tt;
    };
    auto store = [&](int buf) {
        float* da = as + buf * GL_FT * GL_AP + arow * GL_AP + ak;
        da[0] = sa[0];
        da[1] = sa[1];
        float* db = bs + buf * GL_ISLICE;
#pragma unroll
        for (int n = 0; n < 2; ++n) *(f32x4*)(db + 4 * (n * GL_WG + tid)) = sb[n];
    };
    load(0);
    store(0);
    __syncthreads();

    const int total = a.ntt * a.nks;
    f32x16 acc;
    int buf = 0;
    for (int q = 0; q < total; ++q) {
        const int tt = q / a.nks, ks = q - tt * a.nks;
        const bool more = q + 1 < total;
        if (more) load(q + 1);
        if (ks == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        }
        const float* ap = as + buf * GL_FT * GL_AP + i * GL_AP + h;
        const float* bp = bs + buf * GL_ISLICE + h * GL_FQ + w * 32 + i;
#pragma unroll
        for (int s = 0; s < GL_KS / 2; ++s)              // entries 2 s + h of the slice
            acc = mfma_f32_32x32x2(ap[2 * s], bp[2 * s * GL_FQ], acc);
        if (more) store(buf ^ 1);
        const int n = tt * GL_FQ + w * 32 + i;
        if (ks == a.nks - 1 && n < a.win) {
#pragma unroll
            for (int r = 0; r < 16; ++r) fr[((r & 3) + 8 * (r >> 2) + 4 * h) * a.win + n] = acc[r];
        }
        __syncthreads();             // slice q + 1 is complete, nobody reads slice q any more; after the last: fr is complete
        buf ^= 1;
    }

    for (int e = tid; e < owned; e += GL_WG) {
        const long u = u0 + e, j = u - a.c;
        if (j < 0 || j >= a.Lout) continue;
        float v = 0.f;
        if (j < Lb) {
            long lo = u - a.win + 1;
            lo = lo <= 0 ? 0 : (lo + a.hop - 1) / a.hop;
            long hi = u / a.hop;
            if (hi > Tb - 1) hi = Tb - 1;
            float env = 0.f;
            for (long t = lo; t <= hi; ++t) {            // (tq <= lo: the halo reaches every frame that covers u)
                const int n = (int)(u - t * a.hop);
                v = v + fr[(int)(t - tq) * a.win + n];
                env = env + a.wsq[n];
            }
            if (env > FLT_MIN) v = v / env;
        }
        y[j] = v;
    }
}

__global__ __launch_bounds__(GL_CHUNK) void deemphasis_kernel(const float* x, float* y, const int* length, int Lmax, float coef) {
    __shared__ float v[2][GL_CHUNK];
    const int tid = threadIdx.x, b = blockIdx.x;
    int L = length[b];
    L = L < 0 ? 0 : (L > Lmax ? Lmax : L);
    const float* xb = x + (size_t)b * Lmax;
    float* yb = y + (size_t)b * Lmax;
    float carry = 0.f;
    for (int n0 = 0; n0 < L; n0 += GL_CHUNK) {           // (L is the same in every work-item)
        const int n = n0 + tid;
        float mine = n < L ? xb[n] : 0.f;
        if (tid == 0) {
            const float c = coef * carry;
            mine = mine + c;
        }
        int cur = 0;
        v[0][tid] = mine;
        __syncthreads();
        float p = coef;
#pragma unroll
        for (int d = 1; d < GL_CHUNK; d <<= 1) {
            if (tid >= d) {
                const float t = p * v[cur][tid - d];
                mine = mine + t;
            }
            v[cur ^ 1][tid] = mine;
            __syncthreads();
            cur ^= 1;
            p = p * p;
        }
        if (n < L) yb[n] = mine;
        carry = v[cur][GL_CHUNK - 1];
        __syncthreads();             // the carry is read before the next chunk overwrites the buffer
    }
}

extern "C" {

int msmc_stft_tile(int which) {
    return which == 0 ? GL_FT : which == 1 ? GL_FQ : which == 2 ? GL_KS : which == 3 ? GL_CHUNK : 0;
}

int msmc_stft(const float* wav, const int* length, const float* basis, int mode, float* out, const float* mag, float* prev,
              float alpha, int B, int Lmax, int Tmax, int n_fft, int win, int hop, float preemphasis, float ref_level_db,
              float min_level_db, float max_abs_value, int symmetric, msmc_stream stream) {
    if (!wav || !length || !basis || !out) return MSMC_E_SHAPE;
    if (mode < 0 || mode > 2 || (mode == 1 && !mag) || (mode != 1 && (mag || prev))) return MSMC_E_SHAPE;
    if (n_fft < 2 || (n_fft & 1) || win < 1 || win > n_fft || hop < 1) return MSMC_E_SHAPE;
    if (B < 1 || B > 65535 || Tmax < 1 || Lmax <= n_fft / 2) return MSMC_E_SHAPE;
    if (mode == 2 && (!(min_level_db < 0.f) || !(max_abs_value > 0.f))) return MSMC_E_SHAPE;
    StftArgs a;
    a.wav = wav; a.length = length; a.basis = basis; a.mag = mag; a.out = out; a.prev = prev;
    a.mode = mode; a.Lmax = Lmax; a.Tmax = Tmax; a.n_fft = n_fft; a.win = win; a.hop = hop; a.F = n_fft / 2 + 1;
    a.WP = (win + GL_KS - 1) / GL_KS * GL_KS;
    a.nft = (a.F + GL_FQ - 1) / GL_FQ;
    a.P = hop < win ? hop : win;
    const long real = hop < win ? (long)(GL_FT - 1) * hop + win : (long)GL_FT * win;
    const long floats = ((long)(GL_FT - 1) * a.P + a.WP + 3) / 4 * 4;
    const long lds = (floats + 2 * GL_SLICE) * (long)sizeof(float);
    if (lds > GL_LDS_MAX) return MSMC_E_SHAPE;
    a.span_real = (int)real; a.span_floats = (int)floats;
    a.pre = preemphasis; a.alpha = alpha; a.ref_db = ref_level_db; a.min_db = min_level_db; a.max_abs = max_abs_value;
    a.symmetric = symmetric != 0;
    int rc = msmc_allow_lds((const void*)stft_kernel, (int)lds);
    if (rc) return rc;
    const unsigned tiles = (unsigned)((Tmax + GL_FT - 1) / GL_FT);
    MSMC_LAUNCH(stft_kernel, dim3(tiles, (unsigned)B), dim3(GL_WG), (size_t)lds, (msmc_stream_t)stream, a);
    return msmc_check_launch();
}

/* frame positions a workgroup of msmc_istft owns at this geometry (32 less the halo); 0 for a refused geometry */
int msmc_istft_tile(int n_fft, int win, int hop) {
    if (n_fft < 2 || (n_fft & 1) || win < 1 || win > n_fft || hop < 1) return 0;
    const int H = (win + hop - 1) / hop - 1;
    if (H >= GL_FT) return 0;
    const long lds = ((long)GL_FT * win + 2 * GL_FT * GL_AP + 2 * GL_ISLICE) * (long)sizeof(float);
    return lds > GL_LDS_MAX ? 0 : GL_FT - H;
}

int msmc_istft(const float* spec, const int* frames, const float* ibasis, const float* wsq, float* y, int B, int Tmax, int n_fft,
               int win, int hop, msmc_stream stream) {
    if (!spec || !frames || !ibasis || !wsq || !y) return MSMC_E_SHAPE;
    if (B < 1 || B > 65535 || Tmax < 2) return MSMC_E_SHAPE;
    IstftArgs a;
    a.PT = msmc_istft_tile(n_fft, win, hop);
    if (a.PT < 1) return MSMC_E_SHAPE;
    if ((long)hop * (Tmax - 1) + n_fft > 0x7fffffffL) return MSMC_E_SHAPE;
    a.spec = spec; a.frames = frames; a.ibasis = ibasis; a.wsq = wsq; a.y = y;
    a.Tmax = Tmax; a.n_fft = n_fft; a.win = win; a.hop = hop; a.F = n_fft / 2 + 1;
    a.K = 2 * a.F;
    a.nks = (a.K + GL_KS - 1) / GL_KS;
    a.ntt = (win + GL_FQ - 1) / GL_FQ;
    a.H = GL_FT - a.PT;
    a.c = n_fft / 2 - (n_fft - win) / 2;
    a.Lout = hop * (Tmax - 1);
    const long lds = ((long)GL_FT * win + 2 * GL_FT * GL_AP + 2 * GL_ISLICE) * (long)sizeof(float);
    int rc = msmc_allow_lds((const void*)istft_kernel, (int)lds);
    if (rc) return rc;
    const long span = (long)a.PT * hop;
    const unsigned tiles = (unsigned)(((long)a.c + a.Lout + span - 1) / span);
    MSMC_LAUNCH(istft_kernel, dim3(tiles, (unsigned)B), dim3(GL_WG), (size_t)lds, (msmc_stream_t)stream, a);
    return msmc_check_launch();
}

int msmc_deemphasis(const float* x, float* y, const int* length, int B, int Lmax, float coef, msmc_stream stream) {
    if (!x || !y || !length || B < 1 || B > 65535 || Lmax < 1) return MSMC_E_SHAPE;
    MSMC_LAUNCH(deemphasis_kernel, dim3((unsigned)B), dim3(GL_CHUNK), 0, (msmc_stream_t)stream, x, y, length, Lmax, coef);
    return msmc_check_launch();
}

}  // extern "C"
