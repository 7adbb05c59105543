// vq_common.inc -- the arithmetic of the exact nearest-codeword search, defined once (included from vq.hip).
//
// vq_search_kernel, vq_search_reg_kernel (vq.hip) and vq_search_stream_kernel (vq_stream.inc) produce the same bits for the
// same shape because they are built from these pieces; oracle/c/vq_oracle.c mirrors them.  Lane (f, g) = (lane & 15,
// lane >> 4) of a wave works on frame f of the wave's 16-frame tile; the four lane groups g share the frame.  Every multiply
// and add is a statement of its own (-ffp-contract=off): one rounding each.
//   register form : d = 16 * NX, the lane holds x[f][16t + 4g + jj] in xb[t][jj]; channel order (t, jj, g)
//   LDS form      : any d % 4 == 0, the head's slice of frame f at xr[0 .. d-1];   channel order 0 .. d-1, lane group g
//                   taking j = g, g + 4, ...
// Codebook rows sit in LDS at pitch ES = d + 4 floats.

// sum over the four lane groups of a frame: l ^ 16 first, then l ^ 32
MSMC_DEV float vq_group_sum(float v) {
    v = v + wave_xor(v, 16);
    v = v + wave_xor(v, 32);
    return v;
}

// |x|^2: pow(2) then sum -- the square is rounded, then added
template <int NX>
MSMC_DEV float vq_sumsq_reg(const f32x4 (&xb)[NX]) {
    float xx = 0.f;
#pragma unroll
    for (int t = 0; t < NX; ++t)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            float sq = xb[t][jj] * xb[t][jj];
            xx = xx + sq;
        }
    return vq_group_sum(xx);
}
MSMC_DEV float vq_sumsq_lds(const float* xr, int d, int g) {
    float xx = 0.f;
    for (int j = g; j < d; j += 4) {
        float v = xr[j];
        float sq = v * v;
        xx = xx + sq;
    }
    return vq_group_sum(xx);
}

// x . e of 16 frames x 16 codewords on the f32 matrix cores (exact fp32, k-ordered fmaf chain).  a_row: this lane's codeword
// row at its first channel (4g in the register form, g in the LDS form).  The two-tile forms take the next 16 codewords
// (a1 = a0 + 16 rows) along: two independent accumulators cover the 40-cycle dependent latency of the instruction.
template <int NX>
MSMC_DEV void vq_dot_reg(const float* a_row, const f32x4 (&xb)[NX], f32x4& acc) {
#pragma unroll
    for (int t = 0; t < NX; ++t) {
        const f32x4 av = *(const f32x4*)(a_row + 16 * t);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) acc = mfma_f32_16x16x4(av[jj], xb[t][jj], acc);
    }
}
template <int NX>
MSMC_DEV void vq_dot_reg2(const float* a0, const float* a1, const f32x4 (&xb)[NX], f32x4& acc0, f32x4& acc1) {
#pragma unroll
    for (int t = 0; t < NX; ++t) {
        const f32x4 av0 = *(const f32x4*)(a0 + 16 * t);
        const f32x4 av1 = *(const f32x4*)(a1 + 16 * t);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            acc0 = mfma_f32_16x16x4(av0[jj], xb[t][jj], acc0);
            acc1 = mfma_f32_16x16x4(av1[jj], xb[t][jj], acc1);
        }
    }
}
MSMC_DEV void vq_dot_lds(const float* a_row, const float* b, int d, f32x4& acc) {
    for (int s = 0; s < d; s += 4) acc = mfma_f32_16x16x4(a_row[s], b[s], acc);
}
MSMC_DEV void vq_dot_lds2(const float* a0, const float* a1, const float* b, int d, f32x4& acc0, f32x4& acc1) {
    for (int s = 0; s < d; s += 4) {
        float bv = b[s];
        acc0 = mfma_f32_16x16x4(a0[s], bv, acc0);
        acc1 = mfma_f32_16x16x4(a1[s], bv, acc1);
    }
}

// the lane's four distances of an accumulator fragment (codewords code0 .. code0 + 3, their norms at en_tile) against its
// running minimum: ascending, a later codeword wins only on a strictly smaller distance
MSMC_DEV void vq_take_min(const f32x4& acc, float xx, const float* en_tile, int code0, float& best, int& bi) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float t2 = 2.f * acc[r];
        float dist = (xx - t2) + en_tile[r];
        if (dist < best) { best = dist; bi = code0 + r; }
    }
}

// first minimum across the four lane groups that share a frame: the smaller index wins a tie
MSMC_DEV void vq_merge_groups(float& best, int& bi) {
#pragma unroll
    for (int m = 16; m <= 32; m <<= 1) {
        float od = wave_xor(best, m);
        int oi = wave_xor(bi, m);
        if (od < best || (od == best && oi < bi)) { best = od; bi = oi; }
    }
}

// straight-through value o = x + (q - x) and the squared error summed over the heads.  first: head 0 starts the sum; the
// place prev comes from may hold no value yet then (the LDS kernel's dacc row): such a caller passes first ? 0.f : <place>.
MSMC_DEV void vq_st(float q, float x, float prev, bool first, float& o, float& s) {
    float e = q - x;
    o = x + e;
    float sq = e * e;
    s = first ? sq : (prev + sq);
}
MSMC_DEV void vq_st_piece(const f32x4& q4, const f32x4& x4, const f32x4& prev4, bool first, f32x4& o4, f32x4& s4) {
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        float o, s;
        vq_st(q4[jj], x4[jj], prev4[jj], first, o, s);
        o4[jj] = o;
        s4[jj] = s;
    }
}
// mean over the heads: a division (the reference divides), and none for one head
MSMC_DEV void vq_div_heads(f32x4& v, int H) {
    const float fh = (float)H;
    if (H > 1) { v[0] = v[0] / fh; v[1] = v[1] / fh; v[2] = v[2] / fh; v[3] = v[3] / fh; }
}

// the resident kernels' codebook of heads [h0, h0 + cnt): rows of d floats -> cb at pitch ES, norms -> en (whole workgroup)
MSMC_DEV void vq_stage_heads(float* cb, float* en, const float* embed_t, const float* enorm, int h0, int cnt, int K, int d,
                             int ES) {
    const int rows = cnt * K, dv = d >> 2;
    const f32x4* src = (const f32x4*)(embed_t + (size_t)h0 * K * d);
    for (int e = threadIdx.x; e < rows * dv; e += blockDim.x) {
        int r = e / dv, c4 = e - r * dv;
        *(f32x4*)(cb + (size_t)r * ES + c4 * 4) = src[e];
    }
    for (int e = threadIdx.x; e < rows; e += blockDim.x) en[e] = enorm[(size_t)h0 * K + e];
}
