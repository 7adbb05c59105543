// resample.hip -- waveform preparation for gfx950: downmix, rational resampling and peak normalisation of a padded batch, the
// step every recipe of the reference starts with (examples/csmsc/scripts/audio/audio_normalization.sh:
// `sox in.wav -c 1 -r $sample_rate --norm=-7 out.wav`).  sox's `rate` filter is not reproduced; the algorithm is this tree's
// stated choice, a Kaiser-windowed-sinc polyphase resampler.  Host side: msmctts_amd/hip/resample.py.
//
// DEFINITION.  rate_in -> rate_out, g = gcd(rate_out, rate_in), up = rate_out / g, down = rate_in / g, mx = max(up, down).
//   half = ceil(zeros mx / rolloff), fc = rolloff / mx
//   h[k] = up fc sinc(fc k) kaiser(2 half + 1, beta)[k + half], -half <= k <= half       float64, rounded to fp32 once
//   y[n] = sum_i x[i] h[n down - i up] over the i in [0, L) whose tap exists; x = 0 beyond the ends (no reflection)
//   L_out = ceil(L up / down)
// which is scipy.signal.resample_poly(x, up, down, window=h / up), lengths included.  Presets (resampy's published sets):
// kaiser_best zeros = 64, rolloff = 0.9475937167399596, beta = 14.769656459379492; kaiser_fast 16, 0.85, 8.555504641634386.
// Several channels are averaged first: xbar = (x_0 + ... + x_{C-1}) / C, summed in channel order in fp32, one IEEE division;
// int16 is scaled by 1 / 32768 (exact) before the sum; C == 1 is a plain read.
//
// POLYPHASE FORM.  Write n = q up + p with 0 <= p < up, and p down + half = o_p up + s_p with 0 <= s_p < up.  A tap
// m = n down - i up of output n has m + half = up (q down + o_p - i) + s_p, so with j = q down + o_p - i
//   y[q up + p] = sum_{j = 0}^{P - 1} bank[p][j] x[q down + o_p - j],  bank[p][j] = h[up j + s_p - half] (0 past the filter's end)
// and P = ceil((2 half + 1) / up).  The bank [up][P] is stored by OUTPUT phase p (down is a unit mod up, so p -> s_p permutes the
// filter's phases); the kernel needs only o_p = (p down + half) / up, in int (p down + half < 2^21 within the bounds below).
// Positions are q down + o_p in 64 bits: n down is never formed.
//
// msmc_resample: ONE launch.  A workgroup of 256 owns a slab of PS consecutive output phases and QT consecutive values of q of one
// utterance (grid: q tiles x phase slabs x utterances), because for a fixed phase consecutive q read input positions `down`
// apart with the same taps:
//   - it stages ONE contiguous input span, positions q0 down + o_{p0} - (P - 1) .. (q0 + QT - 1) down + o_{p0 + PS - 1}, into
//     LDS, downmixing and scaling as it goes: no mono copy and no up-sampled signal reaches memory;
//   - it stages only ITS PS rows of the bank (row pitch P | 1 against bank conflicts).  The whole bank need not fit: at
//     44.1 -> 16 kHz (up = 160, P = 373) it is 233 KB, a slab of 32 rows 47 KB;
//   - work-item e of the tile takes outputs e, e + 256, ...: phase p0 + e % PS, q = q0 + e / PS.  Lanes run over the phases
//     first, so the stores n = q up + p are runs of PS consecutive floats, the bank reads are conflict-free and the input reads
//     of a wave fall within a few consecutive words (up > 1) or `down` apart (up == 1);
//   - its outputs at n >= L_out are written as +0 (a tile wholly behind L_out stages nothing), and the largest |y| of its
//     outputs goes to partials[b][slab * qtiles + qtile].
// PS = min(up, 32), halved while PS (P | 1) floats exceed 48 KB; QT = max(1, 1024 / PS), halved while the span exceeds 64 KB.
// Neither changes a sum.  What it lacks for speed: each tap costs two LDS reads per multiply-add; holding several q per
// work-item would share the bank read (profiles/resample.md).
//
// msmc_peak_scale: the second launch.  Every workgroup reduces its utterance's partials (work-item t takes partials t, t + 256,
// ... in ascending order, then a tree over the 256; max does not depend on the order), gain = target / peak, one IEEE division,
// and scales its 4096 samples in place.  peak == 0: untouched.  The peak is taken AFTER the filter, which can raise it.
//
// SUMMATION ORDER (fixed; no atomics; nothing depends on the grid, the batch, Lmax_in or the padding):
//   xbar : v = fl(x_0 s); v = fl(v + fl(x_c s)), c = 1 .. C - 1; xbar = fl(v / float(C)) for C > 1   (s = 1 / 32768 for int16: exact)
//   y[n] : acc = +0; acc = fl(acc + fl(bank[p][j] xbar[q down + o_p - j])), j = 0 .. P - 1; taps outside [0, L) contribute a
//          product with +0 (acc never becomes -0, so they change nothing).  The build does not contract.
//   out  : fl(y fl(target / peak))
//
// Who guarantees what.  THE KERNEL CHECKS: length[b] is clamped to [0, Lmax_in]; an input position is tested against [0, L_b)
// before its address is formed, an output position against Lmax_out; an empty utterance gets a row of zeros.  THE LAUNCHER
// CHECKS: no NULL operand, x_dtype 0 / 1, 1 <= B <= 65535, 1 <= C <= 8, 1 <= up, down <= 1024 and coprime, half >= 0,
// 1 <= P <= 1024 and P == ceil((2 half + 1) / up), Lmax_in >= 1, Lmax_out >= ceil(Lmax_in up / down), Lmax_out < 2^31 - 2^21, the
// grid's y dimension, and the LDS budget (160 KB); MSMC_E_SHAPE launches nothing.  THE CALLER GUARANTEES: the buffers' shapes,
// contiguous, and partials of msmc_resample_parts floats per utterance.
#include <msmc_rt.hpp>
#include <msmc_hip.h>

#define RS_WG 256
#define RS_MAX_RATIO 1024                // up, down
#define RS_MAX_TAPS 1024                 // P
#define RS_PS 32                         // phases of a slab, at most
#define RS_OUT 1024                      // outputs of a tile, about
#define RS_BANK_MAX (48 * 1024)
#define RS_SPAN_MAX (64 * 1024)
#define RS_LDS_MAX (160 * 1024)
#define RS_CHUNK 4096                    // samples a workgroup of msmc_peak_scale scales

struct ResampleArgs {
    const void* x;
    const int* length;
    const float* bank;
    float* y;
    float* part;
    int dtype, Lmax_in, C, Lmax_out, up, down, P, half;
    int PS, QT, PP, span, qtiles, nparts;    // PP: pitch of a bank row in LDS; span: floats of the staged input
};

struct ResampleTile { int PS, QT, PP, span; };

// the tiling of (up, down, P); PS == 0: refused
static ResampleTile resample_tiling(int up, int down, int P) {
    ResampleTile t = {0, 0, 0, 0};
    if (up < 1 || down < 1 || up > RS_MAX_RATIO || down > RS_MAX_RATIO || P < 1 || P > RS_MAX_TAPS) return t;
    t.PP = P | 1;
    t.PS = up < RS_PS ? up : RS_PS;
    while (t.PS > 1 && (long)t.PS * t.PP * (long)sizeof(float) > RS_BANK_MAX) t.PS >>= 1;
    t.QT = RS_OUT / t.PS > 1 ? RS_OUT / t.PS : 1;
    for (;;) {
        // o_{p0 + PS - 1} - o_{p0} <= ((PS - 1) down) / up + 1
        const long span = (long)(t.QT - 1) * down + ((long)(t.PS - 1) * down) / up + 1 + P;
        if (span * (long)sizeof(float) <= RS_SPAN_MAX || t.QT == 1) { t.span = (int)span; break; }
        t.QT >>= 1;
    }
    return t;
}

// the downmixed sample i of a row (i within the utterance)
MSMC_DEV float resample_read(const void* row, long i, int C, int dtype) {
    float v;
    if (dtype == 1) {
        const short* s = (const short*)row + i * C;
        v = (float)s[0] * (1.f / 32768.f);
        for (int c = 1; c < C; ++c) v = v + (float)s[c] * (1.f / 32768.f);
    } else {
        const float* s = (const float*)row + i * C;
        v = s[0];
        for (int c = 1; c < C; ++c) v = v + s[c];
    }
    return C > 1 ? v / (float)C : v;
}

// max over the workgroup of v >= 0, in every work-item; red: RS_WG floats of LDS
MSMC_DEV float resample_block_max(float v, float* red, int tid) {
    red[tid] = v;
    __syncthreads();
    for (int s = RS_WG / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const float o = red[tid + s];
            if (o > red[tid]) red[tid] = o;
        }
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(RS_WG) void resample_kernel(ResampleArgs a) {
    MSMC_DYN_LDS(smem);
    float* red = (float*)smem;                           // [RS_WG]
    float* bk = red + RS_WG;                             // [PS][PP]
    float* xs = bk + a.PS * a.PP;                        // [span]
    const int tid = threadIdx.x;
    const int qt = blockIdx.x, slab = blockIdx.y, b = blockIdx.z;
    int L = a.length[b];
    L = L < 0 ? 0 : (L > a.Lmax_in ? a.Lmax_in : L);
    long Lout = ((long)L * a.up + a.down - 1) / a.down;
    if (Lout > a.Lmax_out) Lout = a.Lmax_out;
    const int p0 = slab * a.PS;
    const int ps = a.up - p0 < a.PS ? a.up - p0 : a.PS;  // live phases of this slab (>= 1 by the grid)
    const long q0 = (long)qt * a.QT;
    float* y = a.y + (size_t)b * a.Lmax_out;
    float* part = a.part + (size_t)b * a.nparts + (size_t)slab * a.qtiles + qt;
    const int cells = ps * a.QT;

    if (q0 * a.up + p0 >= Lout) {                        // (the same in every work-item) nothing but zeros in this tile
        for (int e = tid; e < cells; e += RS_WG) {
            const long n = (q0 + e / ps) * a.up + p0 + e % ps;
            if (n < a.Lmax_out) y[n] = 0.f;
        }
        if (tid == 0) *part = 0.f;
        return;
    }

    const int o_lo = (p0 * a.down + a.half) / a.up;
    const long first = q0 * a.down + o_lo - (a.P - 1);   // the input position of xs[0]
    {
        const char* row = (const char*)a.x + (size_t)b * a.Lmax_in * a.C * (a.dtype == 1 ? sizeof(short) : sizeof(float));
        for (int e = tid; e < a.span; e += RS_WG) {
            const long i = first + e;
            xs[e] = (i >= 0 && i < L) ? resample_read(row, i, a.C, a.dtype) : 0.f;
        }
        for (int e = tid; e < ps * a.P; e += RS_WG) {
            const int r = e / a.P, j = e - r * a.P;
            bk[r * a.PP + j] = a.bank[(size_t)(p0 + r) * a.P + j];
        }
    }
    __syncthreads();

    float peak = 0.f;
    for (int e = tid; e < cells; e += RS_WG) {
        const int ql = e / ps, pl = e - ql * ps;
        const long n = (q0 + ql) * a.up + p0 + pl;
        if (n >= a.Lmax_out) continue;
        float acc = 0.f;
        if (n < Lout) {
            const int o = ((p0 + pl) * a.down + a.half) / a.up;
            const float* h = bk + pl * a.PP;
            const float* x = xs + (ql * a.down + (o - o_lo) + (a.P - 1));       // x[-j]: j <= P - 1 keeps the index >= 0
#pragma unroll 4
            for (int j = 0; j < a.P; ++j) {
                const float t = h[j] * x[-j];
                acc = acc + t;
            }
            const float m = acc < 0.f ? -acc : acc;
            if (m > peak) peak = m;
        }
        y[n] = acc;
    }
    peak = resample_block_max(peak, red, tid);
    if (tid == 0) *part = peak;
}

struct PeakArgs {
    float* y;
    const float* part;
    const int* out_length;
    float* peak;
    int Lmax_out, nparts;
    float target;
};

__global__ __launch_bounds__(RS_WG) void peak_scale_kernel(PeakArgs a) {
    __shared__ float red[RS_WG];
    const int tid = threadIdx.x, b = blockIdx.y;
    const float* part = a.part + (size_t)b * a.nparts;
    float peak = 0.f;
    for (int e = tid; e < a.nparts; e += RS_WG) {
        const float v = part[e];
        if (v > peak) peak = v;
    }
    peak = resample_block_max(peak, red, tid);
    if (a.peak && blockIdx.x == 0 && tid == 0) a.peak[b] = peak;
    if (!(peak > 0.f)) return;
    int L = a.out_length[b];
    L = L < 0 ? 0 : (L > a.Lmax_out ? a.Lmax_out : L);
    const float gain = a.target / peak;
    float* y = a.y + (size_t)b * a.Lmax_out;
    const long n0 = (long)blockIdx.x * RS_CHUNK;
    for (int e = tid; e < RS_CHUNK; e += RS_WG) {
        const long n = n0 + e;
        if (n < L) y[n] = y[n] * gain;
    }
}

static int resample_gcd(int a, int b) {
    while (b) { const int t = a % b; a = b; b = t; }
    return a;
}

extern "C" {

int msmc_resample_tile(int which, int up, int down, int P) {
    const ResampleTile t = resample_tiling(up, down, P);
    return which == 0 ? t.PS : which == 1 ? t.QT : 0;
}

int msmc_resample_parts(int Lmax_out, int up, int down, int P) {
    const ResampleTile t = resample_tiling(up, down, P);
    if (!t.PS || Lmax_out < 1) return 0;
    const long nq = ((long)Lmax_out + up - 1) / up;
    const long parts = ((nq + t.QT - 1) / t.QT) * ((up + t.PS - 1) / t.PS);
    return parts > 0x7fffffffL ? 0 : (int)parts;
}

int msmc_resample(const void* x, int x_dtype, const int* length, const float* bank, float* y, float* partials, int B, int Lmax_in,
                  int C, int Lmax_out, int up, int down, int P, int half, msmc_stream stream) {
    if (!x || !length || !bank || !y || !partials) return MSMC_E_SHAPE;
    if (x_dtype != 0 && x_dtype != 1) return MSMC_E_SHAPE;
    if (B < 1 || B > 65535 || C < 1 || C > 8 || Lmax_in < 1 || Lmax_out < 1 || half < 0) return MSMC_E_SHAPE;
    const ResampleTile t = resample_tiling(up, down, P);
    if (!t.PS || resample_gcd(up, down) != 1) return MSMC_E_SHAPE;
    if ((long)P != (2L * half + 1 + up - 1) / up) return MSMC_E_SHAPE;
    if ((long)Lmax_out < ((long)Lmax_in * up + down - 1) / down || Lmax_out >= 0x7fffffff - (1 << 21)) return MSMC_E_SHAPE;
    const long lds = ((long)RS_WG + (long)t.PS * t.PP + t.span) * (long)sizeof(float);
    if (lds > RS_LDS_MAX) return MSMC_E_SHAPE;
    const long nq = ((long)Lmax_out + up - 1) / up;
    const long qtiles = (nq + t.QT - 1) / t.QT;
    const int slabs = (up + t.PS - 1) / t.PS;
    if (qtiles * slabs > 0x7fffffffL) return MSMC_E_SHAPE;
    ResampleArgs a;
    a.x = x; a.length = length; a.bank = bank; a.y = y; a.part = partials;
    a.dtype = x_dtype; a.Lmax_in = Lmax_in; a.C = C; a.Lmax_out = Lmax_out; a.up = up; a.down = down; a.P = P; a.half = half;
    a.PS = t.PS; a.QT = t.QT; a.PP = t.PP; a.span = t.span; a.qtiles = (int)qtiles; a.nparts = (int)(qtiles * slabs);
    int rc = msmc_allow_lds((const void*)resample_kernel, (int)lds);
    if (rc) return rc;
    MSMC_LAUNCH(resample_kernel, dim3((unsigned)qtiles, (unsigned)slabs, (unsigned)B), dim3(RS_WG), (size_t)lds, (msmc_stream_t)stream, a);
    return msmc_check_launch();
}

int msmc_peak_scale(float* y, const float* partials, const int* out_length, float* peak, int B, int Lmax_out, int nparts, float target,
                    msmc_stream stream) {
    if (!y || !partials || !out_length) return MSMC_E_SHAPE;
    if (B < 1 || B > 65535 || Lmax_out < 1 || nparts < 1 || !(target > 0.f)) return MSMC_E_SHAPE;
    PeakArgs a;
    a.y = y; a.part = partials; a.out_length = out_length; a.peak = peak; a.Lmax_out = Lmax_out; a.nparts = nparts; a.target = target;
    const unsigned chunks = (unsigned)(((long)Lmax_out + RS_CHUNK - 1) / RS_CHUNK);
    MSMC_LAUNCH(peak_scale_kernel, dim3(chunks, (unsigned)B), dim3(RS_WG), 0, (msmc_stream_t)stream, a);
    return msmc_check_launch();
}

}  // extern "C"
