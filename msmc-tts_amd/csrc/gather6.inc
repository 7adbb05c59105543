// gather6.inc -- thin-channel bf16 forward / data-gradient kernel (variant 50; included by conv.hip after gather5.inc).
//
// The early layers of the resolution / period discriminators and their data gradients (reference msmctts/networks/hifigan/discriminator.py:15-154
// DiscriminatorR / DiscriminatorP: 3 x 3 and 5 x 1 convolutions between 4 and 64 channels over 10^5-10^6 pixels) have
// 8, 16 or 32 INPUT channels: a contraction of 72-288 values per output point.  The tile kernels stage halo tiles of
// 16-64 bytes per pixel through LDS between workgroup barriers and reach 5-9 % of the HBM roofline there.
//
// With Cin >= 8 the implicit-GEMM B operand needs no staging at all: a lane of v_mfma_f32_32x32x16_bf16 supplies
// B[k = 8g .. 8g+7][point j], and with k enumerating (tap, input channel) channel-fastest those eight k are EIGHT
// CONSECUTIVE CHANNELS OF ONE TAP -- one aligned 16-byte global load straight into the fragment register (padding points
// load nothing and hold zeros; the 9-fold re-read of a pixel by its neighbours' taps is served by L1 / L2).  The weights
// (<= 64 x 288 values) sit in LDS for the whole workgroup, rows padded to 16 bytes modulo 256 so that the A-fragment
// ds_read_b128 is conflict-free.  A wave owns tiles of 32 lattice points and walks them alone: no barriers after the
// weights are in, no LDS traffic for x, loads of three k-steps in flight before their MFMAs.  Epilogue as the fifth
// generation (permlane swap -> two runs of eight channels per lane, 16-byte stores).
// Cin = 4 / 2: a piece spans two / four taps (8- / 4-byte loads).
// Scope (cv6_plan refuses the rest): bf16, Cin in {2, 4, 8, 16, 32, 64}, Cout <= 64 (runs of eight channels per store; other
// counts element by element), Cin * taps <= 704 and a weight image of at most 96 KB, 0 <= in_slope <= 1 (applied on the loaded fragment).
#define CV6_HEAD 768                                       // bytes of lane tables in front of the weight image
#ifndef CV6_BATCH
#define CV6_BATCH 3                                        // k-steps whose loads are in flight before their MFMAs
#endif
struct Cv6Run {
    int npoints, ntiles;          // lattice points of the whole batch, tiles of 32
    int nsteps;                   // k16 steps (ceil(Cin * taps / 16))
    int pitch;                    // bytes per weight row in LDS
    int nco;                      // 32-channel output blocks (1 or 2)
    int cin, cinsh;               // input channels (2, 4, 8, 16, 32) and log2 of them
    unsigned int m_qpi, m_qw;     // floor(2^32 / divisor) + 1 for the two divisions of a point index
    int dymin, dymax, dxmin, dxmax;   // extremes of the tap offsets: a point whose taps all fall inside the image needs no padding rule
};

MSMC_DEV int cv6_div(int n, int dv, unsigned int m) {
    if (dv == 1) return n;
    unsigned int q = __umulhi((unsigned int)n, m);
    if (q * (unsigned int)dv > (unsigned int)n) --q;
    return (int)q;
}

template <int NCO>
MSMC_DEV void cv6_body(const msmc_conv_desc& d, const Cv6Run& R, const int block, const int nblocks) {
    MSMC_DYN_LDS(smem);
    typedef unsigned short T;
    // Cin >= 8: a 16-byte piece of the contraction is 8 consecutive channels of one tap (g8 = Cin / 8 pieces per tap);
    // Cin = 4 / 2: it spans 2 / 4 taps of ALL their channels (two 8-byte / four 4-byte loads).  Runtime values: members of
    // a grouped call with different channel counts share one grid.
    const int CIN = R.cin, cinsh = R.cinsh;
    const int g8sh = cinsh >= 3 ? cinsh - 3 : 0;                // log2(pieces per tap), Cin >= 8
    int* tapdy = (int*)smem;                                    // [32]
    int* tapdx = tapdy + 32;                                    // [32]
    int* koff = tapdx + 32;                                     // [128] element offset of contraction piece kk from a point's base pixel
    char* wimg = smem + CV6_HEAD;                               // [32 * NCO][pitch]
    const int tid = threadIdx.x, w = wave_uniform(tid >> 6), lane = tid & 63, li = lane & 31, g = lane >> 5;
    const int Cout = d.Cout, ntaps = d.ntaps, pitch = R.pitch;
    const int nk8 = (ntaps * CIN + 7) >> 3;                     // 8-value groups (pieces) of the contraction

    // ---- weights -> LDS once: row co, 16-byte piece kk = (tap, channel group); rows / pieces past the end are zeros
    for (int e = tid; e < 32 * NCO * (pitch >> 4); e += 256) *(u32x4*)(wimg + (size_t)e * 16) = u32x4{0u, 0u, 0u, 0u};
    if (tid < 32) {
        tapdy[tid] = tid < ntaps ? d.tap_dy[tid] : 0;
        tapdx[tid] = tid < ntaps ? d.tap_dx[tid] : 0;
    }
    if (tid < 128) {                                            // (Cin >= 8: piece kk = (tap, channel group); else unused)
        const int t = tid >> g8sh, cg = tid - (t << g8sh);
        koff[tid] = (CIN >= 8 && t < ntaps) ? (((d.tap_dy[t] * d.Win + d.tap_dx[t]) << cinsh) + cg * 8) : 0;
    }
    __syncthreads();
    if (CIN >= 8) {
        for (int e = tid; e < Cout * nk8; e += 256) {
            const int co = e / nk8, kk = e - co * nk8;
            const int t = kk >> g8sh, cg = kk - (t << g8sh);
            const u32x4 v = *(const u32x4*)((const T*)d.w + (((size_t)d.tap_w[t] * Cout + co) << cinsh) + cg * 8);
            *(u32x4*)(wimg + (size_t)co * pitch + kk * 16) = v;
        }
    } else {
        const int kreal = ntaps << cinsh;                       // element-wise: k = tap * Cin + ci
        for (int e = tid; e < Cout * kreal; e += 256) {
            const int co = e / kreal, k = e - co * kreal;
            const int t = k >> cinsh, ci = k - (t << cinsh);
            *(T*)(wimg + (size_t)co * pitch + k * 2) = ((const T*)d.w)[(((size_t)d.tap_w[t] * Cout + co) << cinsh) + ci];
        }
    }
    __syncthreads();

    const T* xg = (const T*)d.x;
    const float slope = d.in_slope;
    const int qpi = d.QH * d.QW;
    const T* mask = (const T*)d.mask_src;
    const T* res = (const T*)d.res;
    const T* res2 = (const T*)d.res2;
    T* out = (T*)d.out;
    const float mslope = d.mask_slope, odiv = d.out_div, oslope = d.out_slope;
    const char* wrow = wimg + (size_t)li * pitch + g * 16;     // this lane's A-fragment row (block 0), piece g of step 0

    for (int tile = block * 4 + w; tile < R.ntiles; tile += nblocks * 4) {
        const int p = tile * 32 + li;
        const bool live = p < R.npoints;
        const int pc = live ? p : R.npoints - 1;
        const int b = cv6_div(pc, qpi, R.m_qpi), q = pc - b * qpi;
        const int qy = cv6_div(q, d.QW, R.m_qw), qx = q - qy * d.QW;
        const int iy0 = d.iy0 + qy * d.isy, ix0 = d.ix0 + qx * d.isx;
        const int xb = b * d.Hin;
        // VALU discipline (SQ counters, round 4: ~800 vector instructions per tile against 6-9 MFMAs, the SIMDs' vector ports 90 %
        // busy): a tile whose 32 points have ALL their taps inside the image -- 95 % of the tiles -- needs no padding rule, no
        // per-tap pixel arithmetic: piece kk of a point sits koff[kk] elements from the point's base pixel (one LDS read and one
        // add per k-step instead of ~30 instructions).  Border tiles (and Cin < 8) keep the general path.
        const bool inside_pt = live && iy0 + R.dymin >= 0 && iy0 + R.dymax < d.Hin && ix0 + R.dxmin >= 0 && ix0 + R.dxmax < d.Win;
        const bool fast = CIN >= 8 && !wave_any(!inside_pt);
        const T* xbase = xg + (long)((xb + iy0) * d.Win + ix0) * CIN;         // (may point before a row: only base + koff is read)
        f32x16 acc[NCO];
#pragma unroll
        for (int c = 0; c < NCO; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
        // this lane's piece of k-step ks: group kk = 2 ks + g -> (tap, channel group)
        auto load_piece = [&](int ks) -> u32x4 {
            const int kk = 2 * ks + g;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (kk >= nk8) return v;
            auto pixel = [&](int t, unsigned int& off) -> bool {         // element offset of tap t's pixel, false = padding
                int iy = iy0 + tapdy[t], ix = ix0 + tapdx[t];
                bool inside = live;
                if (d.pad_mode == 1) {
                    iy = reflect_index(iy, d.Hin);
                    ix = reflect_index(ix, d.Win);
                } else {
                    inside = inside && (iy >= 0) && (iy < d.Hin) && (ix >= 0) && (ix < d.Win);
                }
                off = (unsigned int)(((xb + iy) * d.Win + ix) << cinsh);
                return inside;
            };
            unsigned int off;
            if (CIN >= 8) {
                const int t = kk >> g8sh, cg = kk - (t << g8sh);
                if (pixel(t, off)) v = *(const u32x4*)(xg + (size_t)off + cg * 8);
            } else if (CIN == 4) {
#pragma unroll
                for (int tp = 0; tp < 2; ++tp) {
                    const int t = 2 * kk + tp;
                    if (t < ntaps && pixel(t, off)) {
                        const u32x2 h = *(const u32x2*)(xg + (size_t)off);
                        v[2 * tp] = h[0];
                        v[2 * tp + 1] = h[1];
                    }
                }
            } else {
#pragma unroll
                for (int tp = 0; tp < 4; ++tp) {
                    const int t = 4 * kk + tp;
                    if (t < ntaps && pixel(t, off)) v[tp] = *(const unsigned int*)(xg + (size_t)off);
                }
            }
            return v;
        };
        // three k-steps' loads in flight before their MFMAs; the step count is padded to a multiple of three (zero pieces
        // on both sides: no conditional MFMA, whose accumulator would be copied around the branch)
        for (int s0 = 0; s0 < R.nsteps; s0 += CV6_BATCH) {
            u32x4 xf[CV6_BATCH];
            if (fast) {
#pragma unroll
                for (int u = 0; u < CV6_BATCH; ++u) {
                    const int kk = 2 * (s0 + u) + g;
                    xf[u] = u32x4{0u, 0u, 0u, 0u};
                    if (kk < nk8) xf[u] = *(const u32x4*)(xbase + koff[kk]);
                }
            } else {
#pragma unroll
                for (int u = 0; u < CV6_BATCH; ++u) xf[u] = load_piece(s0 + u);
            }
#pragma unroll
            for (int u = 0; u < CV6_BATCH; ++u) {
                if (slope != 1.f) {
#pragma unroll
                    for (int q4 = 0; q4 < 4; ++q4) xf[u][q4] = bf16x2_leaky(xf[u][q4], slope);
                }
#pragma unroll
                for (int c = 0; c < NCO; ++c) {
                    const u32x4 wf = *(const u32x4*)(wrow + (size_t)c * 32 * pitch + (s0 + u) * 32);
                    acc[c] = mfma_bf16_32x32x16(__builtin_bit_cast(bf16x8, wf), __builtin_bit_cast(bf16x8, xf[u]), acc[c]);
                }
            }
        }
        // ---- epilogue in registers: lane (li, g) owns point p and, after the swap, channels 32 c + 16 h + 8 g + (0 .. 7)
#pragma unroll
        for (int c = 0; c < NCO; ++c) cv5_swap_runs(acc[c]);
        if (!live) continue;
        const size_t opix = ((size_t)b * d.Hout + d.oy0 + qy * d.osy) * d.Wout + d.ox0 + qx * d.osx;
#pragma unroll
        for (int c = 0; c < NCO; ++c) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int n = 32 * c + 16 * h + 8 * g;
                if (n >= Cout) continue;
                const size_t o = opix * Cout + n;
                if (n + 4 == Cout && !(Cout & 3)) {
                    // a last run of FOUR channels (the 8 -> 4 data gradients of the resolution discriminators' first layers: 800 k
                    // points of four channels): 8-byte operand loads and one 8-byte store -- element by element this was four
                    // 2-byte stores and four 2-byte loads per operand and point
                    f32x4 b0 = {0.f, 0.f, 0.f, 0.f};
                    if (d.bias) b0 = *(const f32x4*)(d.bias + n);
                    u32x2 mk = {0u, 0u}, r1 = mk, r2 = mk;
                    if (mask) mk = *(const u32x2*)(mask + o);
                    if (res) r1 = *(const u32x2*)(res + o);
                    if (res2) r2 = *(const u32x2*)(res2 + o);
                    float ov[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) ov[j] = acc[c][8 * h + j] + b0[j];
                    {
                        const unsigned int mkw[2] = {mk[0], mk[1]}, r1w[2] = {r1[0], r1[1]}, r2w[2] = {r2[0], r2[1]};
                        cv_ep<4>(ov, mkw, r1w, r2w, mask != nullptr, res != nullptr, res2 != nullptr, mslope, odiv, oslope);
                    }
                    const u32x2 pk = {pack_bf16x2(ov[0], ov[1]), pack_bf16x2(ov[2], ov[3])};
                    *(u32x2*)(out + o) = pk;
                    continue;
                }
                if (n + 8 > Cout || (Cout & 7)) {               // Cout not a multiple of eight: element by element
                    for (int j = 0; j < 8 && n + j < Cout; ++j) {
                        float v = acc[c][8 * h + j] + (d.bias ? d.bias[n + j] : 0.f);
                        if (mask) v = v * (bf16_bits_to_f32(mask[o + j]) > 0.f ? 1.f : mslope);
                        if (res) v = v + bf16_bits_to_f32(res[o + j]);
                        if (res2) v = bf16_bits_to_f32(res2[o + j]) + v;
                        if (odiv != 1.f) v = v / odiv;
                        if (oslope != 1.f) v = v > 0.f ? v : v * oslope;
                        out[o + j] = f32_to_bf16_bits(v);
                    }
                    continue;
                }
                f32x4 b0 = {0.f, 0.f, 0.f, 0.f}, b1 = b0;
                if (d.bias) {
                    b0 = *(const f32x4*)(d.bias + n);
                    b1 = *(const f32x4*)(d.bias + n + 4);
                }
                u32x4 mk = {0u, 0u, 0u, 0u}, r1 = mk, r2 = mk;
                if (mask) mk = *(const u32x4*)(mask + o);
                if (res) r1 = *(const u32x4*)(res + o);
                if (res2) r2 = *(const u32x4*)(res2 + o);
                // (optional operands: cv_ep, conv.hip -- one wave-uniform branch per operand around all eight values)
                float ov[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) ov[j] = acc[c][8 * h + j] + (j < 4 ? b0[j & 3] : b1[j & 3]);
                {
                    const unsigned int mkw[4] = {mk[0], mk[1], mk[2], mk[3]}, r1w[4] = {r1[0], r1[1], r1[2], r1[3]},
                                       r2w[4] = {r2[0], r2[1], r2[2], r2[3]};
                    cv_ep<8>(ov, mkw, r1w, r2w, mask != nullptr, res != nullptr, res2 != nullptr, mslope, odiv, oslope);
                }
                // (v_cvt_pk_bf16_f32: one instruction per value pair; the bit-level helper costs ~6 per value)
                const u32x4 pk = {pack_bf16x2(ov[0], ov[1]), pack_bf16x2(ov[2], ov[3]), pack_bf16x2(ov[4], ov[5]), pack_bf16x2(ov[6], ov[7])};
                *(u32x4*)(out + o) = pk;
            }
        }
    }
}

template <int NCO>
__global__ __launch_bounds__(256) void conv_gather6_kernel(msmc_conv_desc d, Cv6Run R) {
    cv6_body<NCO>(d, R, (int)blockIdx.x, (int)gridDim.x);
}
struct Cv6GroupArgs {
    int n;
    int first[MSMC_GROUP_MAX + 1];
    msmc_conv_desc d[MSMC_GROUP_MAX];
    Cv6Run R[MSMC_GROUP_MAX];
};
template <int NCO>
__global__ __launch_bounds__(256) void conv_gather6_group_kernel(Cv6GroupArgs a) {
    const int k = cv_group_member(a.first, a.n);
    cv6_body<NCO>(a.d[k], a.R[k], (int)blockIdx.x - a.first[k], a.first[k + 1] - a.first[k]);
}

struct Cv6Plan {
    int applies;
    Cv6Run R;
    size_t lds;
    int blocks;
};
static bool cv6_is_variant(int variant) { return variant == 50; }

static int cv6_plan(const msmc_conv_desc* d, Cv6Plan* pl, int share = 1) {
    pl->applies = 0;
    if (d->dtype != 1 || !cv6_is_variant(d->variant)) return 0;
    if (d->Cin != 2 && d->Cin != 4 && d->Cin != 8 && d->Cin != 16 && d->Cin != 32 && d->Cin != 64) return 0;
    if (d->Cout <= 0 || d->Cout > 64 || d->ntaps <= 0 || d->ntaps > 32 || d->Cin * d->ntaps > 704) return 0;
    if (d->Cin < 8 && ((size_t)d->x & (size_t)(d->Cin * 2 - 1))) return 0;
    if (!(d->in_slope >= 0.f && d->in_slope <= 1.f)) return 0;
    if (((size_t)d->x | (size_t)d->w | (size_t)d->out | (size_t)d->res | (size_t)d->res2 | (size_t)d->mask_src | (size_t)d->bias) & 15)
        return 0;
    const long npoints = (long)d->B * d->QH * d->QW;
    if (npoints <= 0 || npoints >= (1L << 31)) return 0;
    if ((long)d->B * d->Hin * d->Win * d->Cin >= (1L << 31) || (long)d->B * d->Hout * d->Wout * d->Cout >= (1L << 31)) return 0;
    Cv6Run& R = pl->R;
    R.npoints = (int)npoints;
    R.ntiles = (int)((npoints + 31) / 32);
    const int k = d->Cin * d->ntaps;
    R.nsteps = (((k + 15) / 16 + CV6_BATCH - 1) / CV6_BATCH) * CV6_BATCH;      // (padded to whole batches of steps)
    R.pitch = ((R.nsteps * 32 + 255) & ~255) + 16;              // 16 bytes modulo 256: consecutive rows on consecutive slots
    R.nco = d->Cout > 32 ? 2 : 1;
    R.cin = d->Cin;
    R.cinsh = d->Cin == 2 ? 1 : d->Cin == 4 ? 2 : d->Cin == 8 ? 3 : d->Cin == 16 ? 4 : d->Cin == 32 ? 5 : 6;
    R.m_qpi = (unsigned int)((1ULL << 32) / (unsigned long long)((long)d->QH * d->QW)) + 1u;
    R.m_qw = (unsigned int)((1ULL << 32) / (unsigned long long)d->QW) + 1u;
    pl->lds = CV6_HEAD + (size_t)32 * R.nco * R.pitch;
    R.dymin = R.dymax = d->tap_dy[0];
    R.dxmin = R.dxmax = d->tap_dx[0];
    for (int t = 1; t < d->ntaps; ++t) {
        if (d->tap_dy[t] < R.dymin) R.dymin = d->tap_dy[t];
        if (d->tap_dy[t] > R.dymax) R.dymax = d->tap_dy[t];
        if (d->tap_dx[t] < R.dxmin) R.dxmin = d->tap_dx[t];
        if (d->tap_dx[t] > R.dxmax) R.dxmax = d->tap_dx[t];
    }
    if (pl->lds > 96 * 1024) return 0;                          // (at least one more workgroup per CU)
    // workgroups: enough waves to hide the load latency (about four workgroups per CU over the members of a launch),
    // never more than one per four tiles
    long nb = (long)(4 * MSMC_NUM_CU) / (share > 0 ? share : 1);
    const long maxb = (R.ntiles + 3) / 4;
    if (nb > maxb) nb = maxb;
    if (nb < 1) nb = 1;
    pl->blocks = (int)nb;
    pl->applies = 1;
    return 0;
}

// SINGLE (d, R) or GROUP launch of one number of output blocks
static int cv6_dispatch(const Cv6Plan& pl, int blocks, size_t lds, msmc_stream stream, const msmc_conv_desc* d,
                        const Cv6GroupArgs* group) {
    int rc;
#define CV6_GO(KERNEL_, NC_, ...)                                                                                  \
    do {                                                                                                           \
        rc = msmc_allow_lds((const void*)KERNEL_<NC_>, (int)lds);                                                  \
        if (rc) return rc;                                                                                         \
        MSMC_LAUNCH((KERNEL_<NC_>), dim3((unsigned)blocks), dim3(256), lds, (msmc_stream_t)stream, __VA_ARGS__);   \
    } while (0)
    if (!group && pl.R.nco == 1) CV6_GO(conv_gather6_kernel, 1, *d, pl.R);
    else if (!group) CV6_GO(conv_gather6_kernel, 2, *d, pl.R);
    else if (pl.R.nco == 1) CV6_GO(conv_gather6_group_kernel, 1, *group);
    else CV6_GO(conv_gather6_group_kernel, 2, *group);
#undef CV6_GO
    static thread_local char name[64];
    snprintf(name, sizeof(name), "%s<%d>", group ? "conv_gather6_group_kernel" : "conv_gather6_kernel", pl.R.nco);
    msmc_conv_last = msmc_prof_name(name);
    return msmc_check_launch();
}

// one descriptor: 1 = launched, 0 = does not apply, < 0 error
static int cv6_launch(const msmc_conv_desc* d, msmc_stream stream) {
    Cv6Plan pl;
    int rc = cv6_plan(d, &pl);
    if (rc) return rc;
    if (!pl.applies) return 0;
    return cv_launched(cv6_dispatch(pl, pl.blocks, pl.lds, stream, d, nullptr));
}

// members of a grouped call (cv_family_group_launch): one grid per number of output blocks (any mix of channel counts),
// every member planned for its share of the chip
struct Cv6Family {
    typedef Cv6Plan Plan;
    typedef Cv6GroupArgs Args;
    static constexpr int min_members = 1;
    static constexpr bool lone_single = true;
    static bool mine(const msmc_conv_desc* d) { return cv6_is_variant(d->variant); }
    static int plan(const msmc_conv_desc* d, Plan* pl, int share) { return cv6_plan(d, pl, share); }
    static bool same(const Plan& p, const Plan& q) { return p.R.nco == q.R.nco; }
    static int blocks(const Plan& p) { return p.blocks; }
    static int* head(Args& a, int m) { a.n = m; return a.first; }
    static void fill(Args& a, int k, const msmc_conv_desc& d, const Plan& p) {
        a.d[k] = d;
        a.R[k] = p.R;
    }
    static int dispatch(const Plan& p, int blocks, size_t lds, msmc_stream stream, const msmc_conv_desc* d, const Args* group) {
        return cv6_dispatch(p, blocks, lds, stream, d, group);
    }
};
