// bn_common.inc -- row-vector width, Chan merge and lane geometry shared by the channels-last statistics kernels
// (csrc/norm.hip msmc_bn_*, csrc/tdnn.hip msmc_relu_bn_* / msmc_se_* / msmc_asp_*).  Included after <msmc_rt.hpp>.
#pragma once
#include "elem.inc"
// a row moves as 16-byte vectors (el_ldv / el_stv of elem.inc): 4 fp32 or 8 bf16 channels per lane
template <typename T> struct bn_vec { static constexpr int V = 4; };
template <> struct bn_vec<unsigned short> { static constexpr int V = 8; };

// (n, mean, m2) <- (n, mean, m2) merged with (nb, mb, m2b): Chan, Golub & LeVeque
MSMC_DEV void bn_chan(float& n, float& mean, float& m2, float nb, float mb, float m2b) {
    if (nb == 0.f) return;
    const float nt = n + nb, d = mb - mean, f = nb / nt;
    mean = mean + d * f;
    m2 = (m2 + m2b) + d * d * (n * f);
    n = nt;
}
// lane geometry of a workgroup: G lanes per row, R rows in flight, this lane = (rr, cg); lanes with rr >= R idle
struct bn_lanes { int G, R, rr, cg; };
template <int V> MSMC_DEV bn_lanes bn_geometry(int C) {
    bn_lanes l;
    l.G = C / V;
    l.R = 256 / l.G < 32 ? 256 / l.G : 32;
    l.rr = (int)threadIdx.x / l.G;
    l.cg = (int)threadIdx.x - l.rr * l.G;
    return l;
}

// slabs of a pass over N rows: every workgroup of the second launch re-reads all partials (nblk x 2 x C floats) and its own slab
// (N / nblk rows of C elements) -- the two are balanced near nblk = sqrt(N / 2); at most one slab per CU
struct bn_grid { int nblk; long slab; };
static bn_grid bn_slabs(long N) {
    const long cap = MSMC_NUM_CU > 0 ? MSMC_NUM_CU : 1;
    long nb = 1;
    while (nb < cap && (nb + 1) * (nb + 1) * 2 <= N) ++nb;
    bn_grid gr;
    gr.slab = N > 0 ? (N + nb - 1) / nb : 1;
    gr.nblk = N > 0 ? (int)((N + gr.slab - 1) / gr.slab) : 0;
    return gr;
}
static bool bn_shape_ok(long N, int C) { return N >= 0 && N < (1L << 31) && C > 0 && (C % 8) == 0 && C <= 1024; }
// streaming passes (evaluation): slabs sized for the whole chip, no partials to re-read
static bn_grid bn_stream_slabs(long N) {
    const long cap = 8L * MSMC_NUM_CU;
    long nb = (N + 31) / 32;
    if (nb > cap) nb = cap;
    if (nb < 1) nb = 1;
    bn_grid gr;
    gr.slab = (N + nb - 1) / nb;
    gr.nblk = (int)((N + gr.slab - 1) / gr.slab);
    return gr;
}
