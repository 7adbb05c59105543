// features.hip -- acoustic features from waveforms in one launch, for gfx950: the normalised log-mel spectrogram and the frame
// energy that the reference computes per file on the CPU (examples/csmsc/scripts/audio/audio.py: preemphasis :23-24,
// melspectrogram / energy :59-73, _stft_parameters :81-85, _linear_to_mel :95-99, _amp_to_db :114-115, _normalize :122-129).
// Host side: msmctts_amd/hip/features.py (FeatureExtractor builds the two constant matrices); tool: tools/extract_features.py.
//
// msmc_mel_features: wav [B][Lmax] fp32, length [B] (device) -> mel [B][Tmax][M], energy [B][Tmax] (optional), T_b = 1 + L_b / hop:
//   p[0] = y[0], p[n] = y[n] - a y[n - 1]                                        pre-emphasis
//   frame t, tap n (0 <= n < win) = p[reflect(t hop + off + n - n_fft / 2)],      off = (n_fft - win) / 2, reflection at L_b
//   re / im[t][f] = sum_n frame[t][n] basis[n][f]                                 window folded into the basis by the host
//   mag = sqrt(re^2 + im^2), m[t][j] = sum_f mag[t][f] melT[f][j], e[t] = sqrt(sum_f mag^2)
//   mel = clip(normalise(20 log10(max(1e-5, m)) - ref_level_db)), rows t >= T_b: zeros.
// Neither a frame nor a spectrum reaches global memory.
//
// A workgroup of four waves owns FEAT_FT = 32 consecutive frames of one utterance (grid: frame tiles x utterances; a tile at or
// past T_b writes its zero rows and leaves).  Its pre-emphasised, reflected sample span -- (FT - 1) hop + win samples where
// frames overlap (hop < win: 28 KB at 200 / 800, the frames themselves would be 100 KB), FT win otherwise -- is staged in LDS
// once; frame i, tap n is span[i P + n], P = min(hop, win).  The frequencies pass by in tiles of FEAT_FQ = 128, 32 per wave.
// For a tile the taps are cut into slices of FEAT_KS = 16: one slice of the basis, [16 taps][128 cos | 128 -sin] = 16 KB and
// contiguous in the host's layout [tile][tap][256], travels L2 -> registers (issued ahead of the slice's MFMAs) -> the other of
// two LDS buffers (behind them), one workgroup barrier per slice.  A wave runs v_mfma_f32_32x32x2_f32 on (32 frames x 2 taps) x
// (2 taps x 32 frequencies) into one re and one im accumulator: lane (i, h) = (lane & 31, lane >> 5) supplies span[i P + 2 s + h]
// to both.  After a tile's last slice the 32 x 128 magnitudes go through LDS (pitch 129: conflict-free both ways) to
//   * the energy: lane (i, h) of wave w sums the squares of frequencies 16 (2 w + h) .. + 15 of frame i; work-items 0..31 then
//     add the tile's eight partial sums and add that to the frame's running sum;
//   * the mel projection: wave w owns mel columns 32 w .. 32 w + 31 (waves past the padded M idle here), a second
//     v_mfma_f32_32x32x2_f32 of (32 frames x 128 magnitudes) against the tile's rows of melT, read from global memory (L2:
//     328 KB at F = 1025, M = 80), accumulated over all tiles.
// The epilogue turns the mel accumulators into normalised dB and the energy sums into roots.
//
// SUMMATION ORDERS (fixed; an fp32 MFMA is a k-ordered fmaf chain; no atomics; nothing depends on the grid):
//   re, im : taps in ascending order from +0, one fmaf per tap (the zero rows that pad win to whole slices come last).
//   mel    : frequencies in ascending order from +0, one fmaf per frequency, over all tiles (padded frequencies add +0).
//   energy : per tile of 128 frequencies eight partial sums of 16 squares each, ascending from +0 (multiply, then add: the build
//            does not contract); the tile's sum = ((p0 + p1) + ... + p7); running sum = running + tile's sum, tiles ascending.
// A frame's values are functions of its own utterance's samples and length only: frame tiles start at multiples of 32 frames of
// the utterance, so neither the batch nor Lmax changes a bit.
//
// Who guarantees what.  THE KERNEL CHECKS: length[b] is clamped to [0, Lmax]; an utterance with length <= n_fft / 2 (one
// reflection would leave the signal) is all zeros; every sample index is tested against [0, L_b) after the reflection, so no
// address outside the row is formed.  THE LAUNCHER CHECKS: the accepted shapes (n_fft even, 1 <= win <= n_fft, hop >= 1,
// 1 <= M <= 128, Lmax > n_fft / 2, B, Tmax >= 1, B < 65536), min_level_db < 0 < max_abs_value, no NULL operand but energy, and
// that the span fits LDS (160 KB less the 49.5 KB of the other buffers: MSMC_E_SHAPE beyond, e.g. win = 2048 with hop >= 900);
// MSMC_E_SHAPE launches nothing.  THE CALLER GUARANTEES: the buffers' shapes -- basis [ceil(F / 128)][ceil(win / 16) 16][256],
// melT [ceil(F / 128) 128][ceil(M / 32) 32], both zero-padded -- contiguous, 16-byte aligned.
#include <msmc_rt.hpp>
#include <msmc_hip.h>

#define FEAT_FT 32                       // frames per workgroup
#define FEAT_FQ 128                      // frequencies per tile (32 per wave)
#define FEAT_KS 16                       // taps per basis slice
#define FEAT_WG 256
#define FEAT_MAGP (FEAT_FQ + 1)          // pitch of the magnitude tile
#define FEAT_SLICE (FEAT_KS * 2 * FEAT_FQ)
#define FEAT_LDS_MAX (160 * 1024)

struct FeatArgs {
    const float* wav;
    const int* length;
    const float* basis;
    const float* melT;
    float* mel;
    float* energy;
    int Lmax, Tmax, n_fft, win, hop, M;
    int WP, MP, nft;                     // padded taps, padded mel columns, frequency tiles
    int P, span_real, span_floats;       // frame pitch in the span, its samples, its floats in LDS (zeros behind the samples)
    float pre, ref_db, min_db, max_abs;
    int symmetric;
};

// floats of LDS behind the span: two basis slices, the magnitude tile, the energy partials
static constexpr int feat_fixed_floats() { return 2 * FEAT_SLICE + FEAT_FT * FEAT_MAGP + 8 * FEAT_FT; }

// audio.py:114-129 on one mel amplitude
MSMC_DEV float feat_normalise(float m, const FeatArgs& a) {
    const float S = 20.f * log10f(fmaxf(1e-5f, m)) - a.ref_db;
    const float u = (S - a.min_db) / (-a.min_db);
    if (a.symmetric) return fminf(fmaxf((2.f * a.max_abs) * u - a.max_abs, -a.max_abs), a.max_abs);
    return fminf(fmaxf(a.max_abs * u, 0.f), a.max_abs);
}

__global__ __launch_bounds__(FEAT_WG) void mel_features_kernel(FeatArgs a) {
    MSMC_DYN_LDS(smem);
    float* span = (float*)smem;                          // [span_floats]
    float* bs = span + a.span_floats;                    // [2][KS][cos FQ | -sin FQ]
    float* mg = bs + 2 * FEAT_SLICE;                     // [FT][MAGP]
    float* ep = mg + FEAT_FT * FEAT_MAGP;                // [8][FT]
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int i = lane & 31, h = lane >> 5;
    const int b = blockIdx.y, t0 = blockIdx.x * FEAT_FT;
    const int half = a.n_fft >> 1;
    int L = a.length[b];
    L = L < 0 ? 0 : (L > a.Lmax ? a.Lmax : L);
    int Tb = L > half ? 1 + L / a.hop : 0;
    if (Tb > a.Tmax) Tb = a.Tmax;
    float* mel = a.mel + (size_t)b * a.Tmax * a.M;
    float* energy = a.energy ? a.energy + (size_t)b * a.Tmax : nullptr;

    if (t0 >= Tb) {                                      // (the same in every work-item) nothing but zero rows in this tile
        const int rows = a.Tmax - t0 < FEAT_FT ? a.Tmax - t0 : FEAT_FT;
        for (int e = tid; e < rows * a.M; e += FEAT_WG) mel[(size_t)t0 * a.M + e] = 0.f;
        if (energy && tid < rows) energy[t0 + tid] = 0.f;
        return;
    }

    // the tile's samples: reflect the index at 0 and at L, then pre-emphasise at that index
    {
        const float* y = a.wav + (size_t)b * a.Lmax;
        const long first = (long)t0 * a.hop + ((a.n_fft - a.win) >> 1) - half;
        for (int e = tid; e < a.span_floats; e += FEAT_WG) {
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

    const int nks = a.WP / FEAT_KS, total = a.nft * nks;
    f32x4 st[4];                                         // a basis slice in flight: 1024 16-byte pieces over 256 work-items
    auto load = [&](int q) {
        const float* src = a.basis + (size_t)q * FEAT_SLICE;
#pragma unroll
        for (int n = 0; n < 4; ++n) st[n] = *(const f32x4*)(src + 4 * (n * FEAT_WG + tid));
    };
    auto store = [&](int buf) {
        float* dst = bs + buf * FEAT_SLICE;
#pragma unroll
        for (int n = 0; n < 4; ++n) *(f32x4*)(dst + 4 * (n * FEAT_WG + tid)) = st[n];
    };
    load(0);
    store(0);
    __syncthreads();

    f32x16 re, im, ml;
#pragma unroll
    for (int r = 0; r < 16; ++r) ml[r] = 0.f;
    float en = 0.f;
    const bool mel_wave = w * 32 < a.MP;                 // (wave-uniform)
    int buf = 0;
    for (int q = 0; q < total; ++q) {
        const int ft = q / nks, ks = q - ft * nks;
        const bool more = q + 1 < total;
        if (more) load(q + 1);
        if (ks == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) re[r] = im[r] = 0.f;
        }
        const float* ap = span + i * a.P + ks * FEAT_KS + h;
        const float* bp = bs + buf * FEAT_SLICE + h * (2 * FEAT_FQ) + w * 32 + i;
#pragma unroll
        for (int s = 0; s < FEAT_KS / 2; ++s) {          // taps 2 s + h
            const float av = ap[2 * s];
            const float cv = bp[2 * s * (2 * FEAT_FQ)], sv = bp[2 * s * (2 * FEAT_FQ) + FEAT_FQ];
            re = mfma_f32_32x32x2(av, cv, re);
            im = mfma_f32_32x32x2(av, sv, im);
        }
        if (more) store(buf ^ 1);

        if (ks == nks - 1) {                             // the tile's spectrum is complete: magnitudes, energy, mel projection
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
                const float rr = re[r] * re[r], ii = im[r] * im[r];
                mg[row * FEAT_MAGP + w * 32 + i] = sqrtf(rr + ii);
            }
            __syncthreads();
            if (energy) {
                const float* mp = mg + i * FEAT_MAGP + 16 * (2 * w + h);
                float s = 0.f;
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const float sq = mp[j] * mp[j];
                    s = s + sq;
                }
                ep[(2 * w + h) * FEAT_FT + i] = s;
            }
            if (mel_wave) {
                const float* mp = mg + i * FEAT_MAGP + h;
                const float* mb = a.melT + ((size_t)ft * FEAT_FQ + h) * a.MP + w * 32 + i;
#pragma unroll 8
                for (int s = 0; s < FEAT_FQ / 2; ++s) ml = mfma_f32_32x32x2(mp[2 * s], mb[(size_t)(2 * s) * a.MP], ml);
            }
            __syncthreads();
            if (energy && tid < FEAT_FT) {
                float s = ep[tid];
#pragma unroll
                for (int p = 1; p < 8; ++p) s = s + ep[p * FEAT_FT + tid];
                en = en + s;
            }
        }
        __syncthreads();             // slice q + 1 is complete, and nobody reads slice q any more
        buf ^= 1;
    }

    if (mel_wave) {
        const int m = w * 32 + i;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int t = t0 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (t < a.Tmax && m < a.M) mel[(size_t)t * a.M + m] = t < Tb ? feat_normalise(ml[r], a) : 0.f;
        }
    }
    if (energy && tid < FEAT_FT && t0 + tid < a.Tmax) energy[t0 + tid] = t0 + tid < Tb ? sqrtf(en) : 0.f;
}

extern "C" {

int msmc_mel_features_tile(int which) { return which == 0 ? FEAT_FT : which == 1 ? FEAT_FQ : which == 2 ? FEAT_KS : 0; }

int msmc_mel_features(const float* wav, const int* length, const float* basis, const float* melT, float* mel, float* energy,
                      int B, int Lmax, int Tmax, int n_fft, int win, int hop, int M, float preemphasis, float ref_level_db,
                      float min_level_db, float max_abs_value, int symmetric, msmc_stream stream) {
    if (!wav || !length || !basis || !melT || !mel) return MSMC_E_SHAPE;
    if (n_fft < 2 || (n_fft & 1) || win < 1 || win > n_fft || hop < 1 || M < 1 || M > 128) return MSMC_E_SHAPE;
    if (B < 1 || B > 65535 || Tmax < 1 || Lmax <= n_fft / 2) return MSMC_E_SHAPE;
    if (!(min_level_db < 0.f) || !(max_abs_value > 0.f)) return MSMC_E_SHAPE;
    FeatArgs a;
    a.wav = wav; a.length = length; a.basis = basis; a.melT = melT; a.mel = mel; a.energy = energy;
    a.Lmax = Lmax; a.Tmax = Tmax; a.n_fft = n_fft; a.win = win; a.hop = hop; a.M = M;
    a.WP = (win + FEAT_KS - 1) / FEAT_KS * FEAT_KS;
    a.MP = (M + 31) / 32 * 32;
    a.nft = (n_fft / 2 + 1 + FEAT_FQ - 1) / FEAT_FQ;
    a.P = hop < win ? hop : win;
    const long real = hop < win ? (long)(FEAT_FT - 1) * hop + win : (long)FEAT_FT * win;
    const long floats = ((long)(FEAT_FT - 1) * a.P + a.WP + 3) / 4 * 4;
    const long lds = (floats + feat_fixed_floats()) * (long)sizeof(float);
    if (lds > FEAT_LDS_MAX) return MSMC_E_SHAPE;
    a.span_real = (int)real; a.span_floats = (int)floats;
    a.pre = preemphasis; a.ref_db = ref_level_db; a.min_db = min_level_db; a.max_abs = max_abs_value;
    a.symmetric = symmetric != 0;
    int rc = msmc_allow_lds((const void*)mel_features_kernel, (int)lds);
    if (rc) return rc;
    const unsigned tiles = (unsigned)((Tmax + FEAT_FT - 1) / FEAT_FT);
    MSMC_LAUNCH(mel_features_kernel, dim3(tiles, (unsigned)B), dim3(FEAT_WG), (size_t)lds, (msmc_stream_t)stream, a);
    return msmc_check_launch();
}

}  // extern "C"
