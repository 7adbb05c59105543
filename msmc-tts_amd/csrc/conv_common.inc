// conv_common.inc -- element access, lattice geometry, kernel naming and the launch bookkeeping shared by the convolution
// units (csrc/conv.hip forward / data gradient, csrc/conv_wgrad.hip weight gradient) and, for Elt<> / cv_group_member / the
// group size, csrc/wnorm.hip.  Included after <msmc_rt.hpp> and <msmc_hip.h>.
#pragma once
#include <cstdio>
#include "elem.inc"

#define CV_BM 128

// Process state both convolution units read: one object each in the library (inline), not part of its ABI (hidden); each
// one's extern "C" setter or getter is in conv.hip.
#define CV_SHARED __attribute__((visibility("hidden"))) inline
// A/B switch (msmc_conv_set_pipeline): 0 = simple kernel, 1 = pipelined kernel with automatic M-tile width,
// 2 / 4 = pipelined kernel forced to 256- / 512-point M tiles (tests).
CV_SHARED int msmc_conv_pipeline_enabled = 1;
// name of the kernel the most recent msmc_conv_gather / msmc_conv_wgrad call of this thread launched (profiling aid:
// bench.py attributes its per-launch HIP-event timings to the same symbols rocprofv3 reports)
CV_SHARED thread_local const char* msmc_conv_last = "";
CV_SHARED thread_local long msmc_conv_launches = 0;          // kernels launched by this thread's gather / wgrad calls
CV_SHARED int msmc_conv_grouping = 1;              // 0: grouped entry points launch their members one by one (A/B)
template <typename T> struct EltName;
template <> struct EltName<float> { static constexpr const char* v = "float"; };
template <> struct EltName<unsigned short> { static constexpr const char* v = "unsigned short"; };
static const char* msmc_kname2(const char* base, const char* elt, int a, int b, int c) {
    static thread_local char buf[96];
    snprintf(buf, sizeof(buf), "%s<%s, %d, %d, %d>", base, elt, a, b, c);
    return buf;
}
static const char* msmc_kname(const char* base, const char* elt, int a, int b) {
    static thread_local char buf[96];
    if (b >= 0 && !elt) snprintf(buf, sizeof(buf), "%s<%d, %d>", base, a, b);
    else if (b >= 0) snprintf(buf, sizeof(buf), "%s<%s, %d, %d>", base, elt, a, b);
    else if (elt) snprintf(buf, sizeof(buf), "%s<%s, %d>", base, elt, a);
    else snprintf(buf, sizeof(buf), "%s<%d>", base, a);
    return buf;
}
#define MSMC_GROUP_LIMIT 16         // members one grouped call may carry (split into launches of <= MSMC_GROUP_MAX)
#define MSMC_GROUP_MAX 6            // members of one grouped launch (CvGroupArgs, conv.hip, says why a grid is shared)
// a descriptor any entry point accepts
static bool cv_desc_ok(const msmc_conv_desc* d) { return d->B > 0 && d->Cin > 0 && d->Cout > 0 && d->QH > 0 && d->QW > 0; }
// result of a one-descriptor family launcher from the status of its launch: 1 = launched, < 0 error (0, does not apply, is
// the launcher's own answer)
static int cv_launched(int rc) { return rc ? (rc < 0 ? rc : -rc) : 1; }

template <typename T> struct Elt {      // float, or unsigned short (bf16 bits): el_ld / el_st of elem.inc take nothing else
    static constexpr int VEC = 16 / (int)sizeof(T);     // elements per 16 bytes
    static constexpr int CK = 64 / (int)sizeof(T);      // channels per 64-byte chunk
    static MSMC_DEV_INLINE float ld(const T* p) { return el_ld(p); }
    static MSMC_DEV_INLINE void st(T* p, float v) { el_st(p, v); }
};

MSMC_DEV int reflect_index(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    if (i < 0) i = 0;
    if (i >= n) i = n - 1;
    return i;
}

struct CvGeom {
    int TH, TW, IH, IW, dyMin, dxMin, tilesX, tilesY, xt_elems;
};

MSMC_DEV int cv_group_member(const int* first, int n) {
    int k = 0;
    while (k + 1 < n && (int)blockIdx.x >= first[k + 1]) ++k;
    return k;
}

static int cv_geometry(const msmc_conv_desc* d, CvGeom* G, int elt_bytes, int XS, int BN, size_t* lds,
                       int bm = CV_BM) {
    if (d->ntaps <= 0 || d->ntaps > MSMC_CONV_MAX_TAPS) return MSMC_E_SHAPE;
    int dyMin = d->tap_dy[0], dyMax = d->tap_dy[0], dxMin = d->tap_dx[0], dxMax = d->tap_dx[0];
    for (int t = 1; t < d->ntaps; ++t) {
        if (d->tap_dy[t] < dyMin) dyMin = d->tap_dy[t];
        if (d->tap_dy[t] > dyMax) dyMax = d->tap_dy[t];
        if (d->tap_dx[t] < dxMin) dxMin = d->tap_dx[t];
        if (d->tap_dx[t] > dxMax) dxMax = d->tap_dx[t];
    }
    int TH, TW;
    if (d->QH == 1) { TH = 1; TW = bm; }
    else if (d->QW <= 16) { TW = d->QW; TH = bm / TW; if (TH < 1) TH = 1; }
    else { TW = 16; TH = bm / 16; }
    G->TH = TH; G->TW = TW;
    G->dyMin = dyMin; G->dxMin = dxMin;
    G->IH = (TH - 1) * d->isy + (dyMax - dyMin) + 1;
    G->IW = (TW - 1) * d->isx + (dxMax - dxMin) + 1;
    G->tilesY = (d->QH + TH - 1) / TH;
    G->tilesX = (d->QW + TW - 1) / TW;
    G->xt_elems = G->IH * G->IW * XS;
    *lds = ((size_t)G->xt_elems + (size_t)d->ntaps * BN * XS) * elt_bytes;
    return 0;
}
