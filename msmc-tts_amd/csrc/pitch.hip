// pitch.hip -- YIN log-F0 tracks from waveforms in one launch, for gfx950, on the frame grid of features.hip (T_b = 1 + L_b / hop,
// frame t centred on sample t hop), so that mel, energy and pitch line up row for row.  The reference ships no F0 tracker; it
// fixes only the convention of the track (utils/audio.py lf02sinexi / lf02peakexi: natural-log F0 on voiced frames, a value <= 0
// on unvoiced ones).  The algorithm is YIN, steps 1-5 (de Cheveigne & Kawahara 2002).  Host side: msmctts_amd/hip/pitch.py.
//
// msmc_pitch_yin: wav [B][Lmax] fp32, length [B] (device) -> pitch [B][Tmax] and, each optional, voiced [B][Tmax] uint8,
// aperiodicity [B][Tmax], cmnd [B][Tmax][tau_max + 2].  With span = W + tau_max + 1 and no pre-emphasis:
//   x_t[j]  = y[reflect(t hop - span / 2 + j)], 0 <= j < span                    reflection at 0 and at L_b
//   d(0)    = 0, d(tau) = sum_{j < W} (x_t[j] - x_t[j + tau])^2, 1 <= tau <= tau_max + 1      the direct difference form
//   S(tau)  = sum_{k = 1..tau} d(k);  d'(0) = 1, d'(tau) = d(tau) tau / S(tau), 1 where S(tau) = 0
//   lag     = the first tau in [tau_min, tau_max] with d'(tau) < threshold, walked up while tau + 1 <= tau_max and
//             d'(tau + 1) < d'(tau); no such tau: the frame is unvoiced
//   delta   = (a - c) / (a - 2 b + c) / 2 clipped to [-1, 1], a, b, c = d'(lag - 1), d'(lag), d'(lag + 1); 0 unless a - 2 b + c > 0
//   pitch   = ln(sr / (lag + delta)) (or the Hz value) on voiced frames, +0 on unvoiced ones and on rows t >= T_b
//   aperiodicity = d'(lag) on voiced frames, min over [tau_min, tau_max] of d' on unvoiced ones; cmnd = the whole d' row.
// No frame reaches global memory.
//
// A workgroup of eight waves owns PITCH_FT = 32 consecutive frames of one utterance (grid: frame tiles x utterances; a tile at or
// past T_b writes its zero rows and leaves).  Its reflected sample span, (FT - 1) hop + span floats (29 KB at 200 / 800 / 266; the
// frames themselves would be 137 KB), is staged in LDS once; x_t[j] of the tile's frame i is xs[i hop + j].
//   A  wave w takes frames w, w + 8, ... of the tile.  Lags map to lanes: in lag block c lane l holds tau = 1 + 64 c + l (lanes past
//      tau_max + 1 repeat that last lag and drop their result), four lag blocks at a time.  For a fixed j the read of x[j] is one
//      address for the whole wave (a broadcast) and x[j + tau] is consecutive across the lanes: ds_read_b32 without bank
//      conflicts, five reads for four lags.  d goes to the frame's row dl[i][tau] in LDS (odd pitch).
//   B  after a workgroup barrier work-item i < 32 walks frame i's row once: running sum S, d' written over d, and the decision
//      (threshold crossing, walk to the local minimum, minimum over the range) as it goes; then the parabola and the outputs.
//   C  after a second barrier the waves copy the d' rows to cmnd, where asked for.
//
// SUMMATION ORDERS (fixed; no atomics; nothing depends on the grid, the batch or Lmax):
//   d(tau) : j ascending from +0; per j one subtraction, one multiply, one add (the build does not contract: three roundings).
//   S(tau) : S(tau) = S(tau - 1) + d(tau), tau ascending from S(0) = +0.
//   d'     : (d(tau) * float(tau)) / S(tau): multiply, then an IEEE division.
//   delta  : num = a - c;  den = (a - (b + b)) + c;  delta = 0.5f * (num / den), then the clip.
//   pitch  : f0 = float(sr) / (float(lag) + delta);  logf(f0).
// Frame tiles start at multiples of 32 frames of the utterance, so an utterance's rows do not depend on its neighbours.
//
// Who guarantees what.  THE KERNEL CHECKS: length[b] is clamped to [0, Lmax]; an utterance with length <= span / 2 is all zeros;
// a sample index is reflected at 0, at L_b and at 0 again and then tested against [0, L_b), so no address outside the row is
// formed.  THE LAUNCHER CHECKS: no NULL operand but the three optional outputs, W, hop, Tmax >= 1, 1 <= B < 65536,
// 2 <= tau_min < tau_max, sample_rate >= 1, threshold > 0, Lmax > span / 2, and that the span and the d rows fit LDS
// (((FT - 1) hop + span + FT ((tau_max + 2) | 1)) floats within 160 KB); MSMC_E_SHAPE launches nothing.  THE CALLER GUARANTEES:
// the buffers' shapes, contiguous.
#include <msmc_rt.hpp>
#include <msmc_hip.h>

#define PITCH_FT 32                      // frames per workgroup
#define PITCH_WG 512
#define PITCH_WAVES (PITCH_WG / MSMC_WAVE)
#define PITCH_LB 4                       // lag blocks of 64 held by a lane at a time
#define PITCH_LDS_MAX (160 * 1024)

struct PitchArgs {
    const float* wav;
    const int* length;
    float* pitch;
    unsigned char* voiced;
    float* aper;
    float* cmnd;
    int Lmax, Tmax, W, hop, tau_min, tau_max;
    int span, span_floats, DP;           // samples of a frame with its lags, floats of the tile's span, pitch of a d row
    float sr, threshold;
    int log;
};

// d(tau) of R lag blocks from block c0 on, for the frame whose samples start at xs: lane l of block c0 + r holds tau = 1 + 64 (c0 + r) + l
template <int R>
MSMC_DEV void pitch_diff(const float* xs, float* row, int c0, int lane, int W, int nlag) {
    const float* p[R];
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int tau = 1 + MSMC_WAVE * (c0 + r) + lane;
        p[r] = xs + (tau < nlag ? tau : nlag);
        acc[r] = 0.f;
    }
#pragma unroll 8
    for (int j = 0; j < W; ++j) {
        const float x = xs[j];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float df = x - p[r][j];
            const float sq = df * df;
            acc[r] = acc[r] + sq;
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int tau = 1 + MSMC_WAVE * (c0 + r) + lane;
        if (tau <= nlag) row[tau] = acc[r];
    }
}

__global__ __launch_bounds__(PITCH_WG) void pitch_yin_kernel(PitchArgs a) {
    MSMC_DYN_LDS(smem);
    float* xs = (float*)smem;                            // [span_floats]
    float* dl = xs + a.span_floats;                      // [FT][DP]
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int b = blockIdx.y, t0 = blockIdx.x * PITCH_FT;
    const int half = a.span >> 1, nlag = a.tau_max + 1, NC = a.tau_max + 2;
    int L = a.length[b];
    L = L < 0 ? 0 : (L > a.Lmax ? a.Lmax : L);
    int Tb = L > half ? 1 + L / a.hop : 0;
    if (Tb > a.Tmax) Tb = a.Tmax;
    const size_t row0 = (size_t)b * a.Tmax;
    const int rows = a.Tmax - t0 < PITCH_FT ? a.Tmax - t0 : PITCH_FT;            // rows of the outputs this tile owns
    const int live = Tb - t0 < rows ? Tb - t0 : rows;                            // of which frames of the utterance

    if (live <= 0) {                                     // (the same in every work-item) nothing but zero rows in this tile
        if (tid < rows) {
            a.pitch[row0 + t0 + tid] = 0.f;
            if (a.voiced) a.voiced[row0 + t0 + tid] = 0;
            if (a.aper) a.aper[row0 + t0 + tid] = 0.f;
        }
        if (a.cmnd)
            for (int e = tid; e < rows * NC; e += PITCH_WG) a.cmnd[(row0 + t0) * NC + e] = 0.f;
        return;
    }

    // the tile's samples: reflect the index at 0, at L and at 0 again (span odd, L = span / 2 + 1), then test it
    {
        const float* y = a.wav + (size_t)b * a.Lmax;
        const long first = (long)t0 * a.hop - half;
        const int need = (live - 1) * a.hop + a.span;
        for (int e = tid; e < need; e += PITCH_WG) {
            long j = first + e;
            if (j < 0) j = -j;
            if (j >= L) j = 2 * ((long)L - 1) - j;
            if (j < 0) j = -j;
            xs[e] = (j >= 0 && j < L) ? y[j] : 0.f;
        }
    }
    __syncthreads();

    // A: the difference function, lags on lanes
    const int nblk = (nlag + MSMC_WAVE - 1) / MSMC_WAVE;
    for (int i = w; i < live; i += PITCH_WAVES) {        // (wave-uniform)
        const float* xf = xs + i * a.hop;
        float* row = dl + i * a.DP;
        int c = 0;
        for (; c + PITCH_LB <= nblk; c += PITCH_LB) pitch_diff<PITCH_LB>(xf, row, c, lane, a.W, nlag);
        const int rest = nblk - c;
        if (rest == 3) pitch_diff<3>(xf, row, c, lane, a.W, nlag);
        else if (rest == 2) pitch_diff<2>(xf, row, c, lane, a.W, nlag);
        else if (rest == 1) pitch_diff<1>(xf, row, c, lane, a.W, nlag);
    }
    __syncthreads();

    // B: one work-item per frame: S, d' in place of d, the decision
    if (tid < rows) {
        float f0 = 0.f, ap = 0.f;
        int voiced = 0;
        if (tid < live) {
            float* row = dl + tid * a.DP;
            row[0] = 1.f;
            float S = 0.f, best = 0.f, lowest = 0.f;
            int lag = 0, state = 0;                      // 0: looking for the crossing, 1: walking down, 2: settled
            for (int tau = 1; tau <= nlag; ++tau) {
                const float d = row[tau];
                S = S + d;
                const float dt = d * (float)tau;
                const float v = S > 0.f ? dt / S : 1.f;
                row[tau] = v;
                if (tau >= a.tau_min && tau <= a.tau_max) {
                    if (tau == a.tau_min || v < lowest) lowest = v;
                    if (state == 0) {
                        if (v < a.threshold) { lag = tau; best = v; state = 1; }
                    } else if (state == 1) {
                        if (v < best) { lag = tau; best = v; }
                        else state = 2;
                    }
                }
            }
            ap = lowest;
            if (lag > 0) {
                const float pa = row[lag - 1], pb = row[lag], pc = row[lag + 1];
                const float num = pa - pc;
                const float den = (pa - (pb + pb)) + pc;
                float delta = 0.f;
                if (den > 0.f) {
                    delta = 0.5f * (num / den);
                    delta = delta < -1.f ? -1.f : (delta > 1.f ? 1.f : delta);
                }
                f0 = a.sr / ((float)lag + delta);
                if (a.log) f0 = logf(f0);
                voiced = 1;
                ap = pb;
            }
        }
        a.pitch[row0 + t0 + tid] = f0;
        if (a.voiced) a.voiced[row0 + t0 + tid] = (unsigned char)voiced;
        if (a.aper) a.aper[row0 + t0 + tid] = ap;
    }
    if (!a.cmnd) return;
    __syncthreads();

    // C: the d' rows
    for (int i = w; i < rows; i += PITCH_WAVES) {
        float* out = a.cmnd + (row0 + t0 + i) * NC;
        const float* row = dl + i * a.DP;
        for (int tau = lane; tau < NC; tau += MSMC_WAVE) out[tau] = i < live ? row[tau] : 0.f;
    }
}

extern "C" {

int msmc_pitch_yin_tile(int which) { return which == 0 ? PITCH_FT : which == 1 ? MSMC_WAVE * PITCH_LB : 0; }

int msmc_pitch_yin(const float* wav, const int* length, float* pitch, unsigned char* voiced, float* aperiodicity, float* cmnd,
                   int B, int Lmax, int Tmax, int W, int hop, int tau_min, int tau_max, int sample_rate, float threshold,
                   int log_f0, msmc_stream stream) {
    if (!wav || !length || !pitch) return MSMC_E_SHAPE;
    if (W < 1 || hop < 1 || Tmax < 1 || B < 1 || B > 65535 || sample_rate < 1) return MSMC_E_SHAPE;
    if (tau_min < 2 || tau_max <= tau_min || !(threshold > 0.f)) return MSMC_E_SHAPE;
    const long span = (long)W + tau_max + 1;
    if ((long)Lmax <= span / 2) return MSMC_E_SHAPE;
    const long DP = (tau_max + 2) | 1;
    const long floats = ((long)(PITCH_FT - 1) * hop + span + 3) / 4 * 4;
    const long lds = (floats + PITCH_FT * DP) * (long)sizeof(float);
    if (lds > PITCH_LDS_MAX) return MSMC_E_SHAPE;
    PitchArgs a;
    a.wav = wav; a.length = length; a.pitch = pitch; a.voiced = voiced; a.aper = aperiodicity; a.cmnd = cmnd;
    a.Lmax = Lmax; a.Tmax = Tmax; a.W = W; a.hop = hop; a.tau_min = tau_min; a.tau_max = tau_max;
    a.span = (int)span; a.span_floats = (int)floats; a.DP = (int)DP;
    a.sr = (float)sample_rate; a.threshold = threshold; a.log = log_f0 != 0;
    int rc = msmc_allow_lds((const void*)pitch_yin_kernel, (int)lds);
    if (rc) return rc;
    const unsigned tiles = (unsigned)((Tmax + PITCH_FT - 1) / PITCH_FT);
    MSMC_LAUNCH(pitch_yin_kernel, dim3(tiles, (unsigned)B), dim3(PITCH_WG), (size_t)lds, (msmc_stream_t)stream, a);
    return msmc_check_launch();
}

}  // extern "C"
