// code_embed.hip -- the per-stage targets of the multi-stage quantiser from stored code indices, for gfx950.  With a frozen
// codebook the quantised output of a stage is, per head, a row of that head's codebook: stage targets (and the predictor's
// teacher-forcing inputs) are a row gather from the prepared codebook embed_t [H][K][d] (hip/vq.py vq_prepare: every codeword
// one contiguous row).  Host side: msmctts_amd/hip/code_embed.py (code_gather); model: MultiStageQuantizer.embed_codes.
//
// msmc_code_gather: out[b][t][h d + c] = embed_t[h][ind[b][t][h]][c] where t < length[b] and 0 <= ind[b][t][h] < K; the d
// channels of a head whose label is outside [0, K), and every row t >= length[b], are +0.  out is fp32 or bf16 (one rounding to
// nearest even, the bits of torch.Tensor.to); ind int32 or int64.  Forward only: the codebook is frozen.
//
// A memory-bound kernel: B T H d elements written, B T H labels read, the codebook (H K d 4 bytes: 512 KB at the shipped
// H = 4, K = 512, d = 64) served from L2.  One work-item per piece of V consecutive channels of one head: V = 4 (fp32 out) or
// V = 8 (bf16 out, d % 8 == 0) make the piece's store 16 bytes, its loads one or two 16-byte accesses (el_ldv / el_stv of
// elem.inc); bf16 out with d % 4 == 0 only takes V = 4 (one 16-byte load, one 8-byte store); any other d, or a pointer off
// its 16-byte boundary, V = 1.  V divides d, so a piece never straddles two heads.  A workgroup of 256 takes CG_PIECES = 2048
// consecutive pieces of the flattened [B T][H d / V] output in two passes of four pieces per work-item -- four labels, then
// four codebook rows in flight, then four stores; a wave stores 1 KB of consecutive bytes per instruction.  Beyond 8 per CU
// workgroups stride over the blocks of pieces (the usual bound for streaming kernels; it keeps the grid inside the launch limit).
//
// Who guarantees what.  THE KERNEL CHECKS: the label range (a label is compared with [0, K) BEFORE it is used to form an address;
// nothing is read for a head whose label fails) and the row's position against length[b] (length may hold anything, negative
// values included: such an utterance is all zeros); every address is formed from indices checked against the buffers' shapes.
// THE LAUNCHER CHECKS: B, T, H, d, K >= 1, the two dtype flags in {0, 1}, no NULL operand (MSMC_E_SHAPE otherwise, nothing
// launched), a row short enough for the 32-bit piece arithmetic (H d / V + CG_PIECES < 2^31), and the alignment that picks V.
// THE CALLER GUARANTEES: the buffers have the stated shapes (ind [B][T][H], length [B], embed_t [H][K][d], out [B][T][H d])
// and are contiguous.
// Every element of out is written exactly once with plain vector stores: no zero-fill launch, no atomics.
#include <msmc_rt.hpp>
#include <msmc_hip.h>
#include "elem.inc"

#define CG_WG 256
#define CG_UNROLL 4
#define CG_PIECES 2048       // pieces per block of rows: two passes of CG_WG x CG_UNROLL

// IT: the labels' type; OT: float or unsigned short (bf16 bits); V: channels per piece; ppr = H d / V pieces per row,
// pph = d / V pieces per head
template <typename IT, typename OT, int V>
__global__ __launch_bounds__(CG_WG) void code_gather_kernel(const IT* __restrict__ ind, const int* __restrict__ length,
                                                           const float* __restrict__ embed_t, OT* __restrict__ out, long pieces,
                                                           long blocks, int T, int H, int d, int K, int ppr, int pph) {
    const int tid = threadIdx.x;
    for (long blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
        // the block's first piece: row n0 = utterance b0, frame t0, piece r0 of the row -- 64-bit divisions once per block (the
        // same in every work-item), 32-bit ones per piece: a piece is fewer than CG_PIECES + ppr pieces behind n0's first
        const long p0 = blk * CG_PIECES;
        const long n0 = p0 / ppr, b0 = n0 / T;
        const unsigned r0 = (unsigned)(p0 - n0 * ppr), t0 = (unsigned)(n0 - b0 * T);
#pragma unroll 1
        for (int pass = 0; pass < CG_PIECES / (CG_WG * CG_UNROLL); ++pass) {
            const unsigned lb = (unsigned)(pass * CG_WG * CG_UNROLL + tid);
            const long pb = p0 + lb;
            long src[CG_UNROLL];                       // the piece's first element in embed_t, -1: zeros
#pragma unroll
            for (int j = 0; j < CG_UNROLL; ++j) {
                const long p = pb + (long)j * CG_WG;
                src[j] = -1;
                if (p < pieces) {
                    const unsigned x = r0 + lb + (unsigned)(j * CG_WG), dn = x / (unsigned)ppr;
                    const unsigned q = x - dn * (unsigned)ppr, h = q / (unsigned)pph, c = (q - h * (unsigned)pph) * V;
                    const unsigned tt = t0 + dn, db = tt / (unsigned)T;
                    const long n = n0 + dn, b = b0 + db;
                    if ((long)(tt - db * (unsigned)T) < (long)length[b]) {
                        const long v = (long)ind[n * H + h];
                        if (v >= 0 && v < K) src[j] = ((long)h * K + v) * d + c;
                    }
                }
            }
            float val[CG_UNROLL][V];
#pragma unroll
            for (int j = 0; j < CG_UNROLL; ++j) {
#pragma unroll
                for (int e = 0; e < V; ++e) val[j][e] = 0.f;
                if (src[j] >= 0) el_ldv<V>(embed_t, src[j], val[j]);
            }
#pragma unroll
            for (int j = 0; j < CG_UNROLL; ++j) {
                const long p = pb + (long)j * CG_WG;
                if (p < pieces) el_stv<V>(out, p * V, val[j]);
            }
        }
    }
}

// channels per piece: 16-byte stores where the width and the alignment allow, else one element
static inline int cg_vec(const float* embed_t, const void* out, int out_bf16, int d) {
    if ((((uintptr_t)embed_t | (uintptr_t)out) & 15) != 0 || d % 4 != 0) return 1;
    return (out_bf16 && d % 8 == 0) ? 8 : 4;
}

extern "C" {

int msmc_code_gather(const void* ind, int ind_i64, const int* length, const float* embed_t, void* out, int out_bf16, int B, int T,
                     int H, int d, int K, msmc_stream stream) {
    if (B < 1 || T < 1 || H < 1 || d < 1 || K < 1) return MSMC_E_SHAPE;
    if (!ind || !length || !embed_t || !out || (ind_i64 | out_bf16) < 0 || ind_i64 > 1 || out_bf16 > 1) return MSMC_E_SHAPE;
    const int V = cg_vec(embed_t, out, out_bf16, d);
    const long ppr = (long)H * d / V;
    if (ppr + CG_PIECES >= 0x7fffffffL) return MSMC_E_SHAPE;
    const long pieces = (long)B * T * ppr, blocks = (pieces + CG_PIECES - 1) / CG_PIECES;
    const long grid = blocks < 8L * MSMC_NUM_CU ? blocks : 8L * MSMC_NUM_CU;
#define CG_GO(IT, OT, VV)                                                                                                       \
    MSMC_LAUNCH((code_gather_kernel<IT, OT, VV>), dim3((unsigned)grid), dim3(CG_WG), 0, (msmc_stream_t)stream, (const IT*)ind, \
                length, embed_t, (OT*)out, pieces, blocks, T, H, d, K, (int)ppr, d / VV)
#define CG_BY_LABEL(OT, VV)                       \
    do {                                          \
        if (ind_i64) CG_GO(int64_t, OT, VV);      \
        else CG_GO(int, OT, VV);                  \
    } while (0)
    if (!out_bf16) {
        if (V == 4) CG_BY_LABEL(float, 4);
        else CG_BY_LABEL(float, 1);
    } else {
        if (V == 8) CG_BY_LABEL(unsigned short, 8);
        else if (V == 4) CG_BY_LABEL(unsigned short, 4);
        else CG_BY_LABEL(unsigned short, 1);
    }
#undef CG_BY_LABEL
#undef CG_GO
    return msmc_check_launch();
}

}  // extern "C"
