/* msmc_hip.h -- C ABI of libmsmc_hip.so, the gfx950 kernels under the msmctts.networks boundary.
 *
 * The reference's drop-in boundary for this path is a Python plugin registry, not an FFI
 * (reference msmctts/networks/__init__.py:6-11).  This library sits *below* it:
 * every entry point takes plain device pointers, sizes and a HIP stream, allocates nothing (msmc_stream_create, which
 * makes a HIP stream, is the one exception), is stream-ordered and re-entrant per stream, and returns 0 (hipSuccess) or a
 * hipError_t / negative MSMC_E* code.  No entry point of this header changes or observes process-global state: kernel choices are
 * per call (msmc_conv_desc.variant / split_shift); the one piece of per-thread state is the sink of msmc_conv_wgrad_defer_begin
 * / _end, armed around single calls.  The A/B switches, ablation masks, the profiling observers (last-kernel tags, launch
 * counter, the msmc_prof_* launch log) that the perf tools, bench.py's kernel table and the tests use live in
 * include/msmc_hip_debug.h, outside the product ABI.  The Python host side (msmc-tts_amd/msmctts_amd) binds these with
 * ctypes from modules that carry the reference's class names; INTEGRATION.md shows the stub a
 * reference maintainer would add.
 *
 * Layout conventions
 *   frames    x        [N][D] fp32 row-major, N = B*T_s frames (padded frames included)
 *   codebook  embed    [H][d][K] fp32 (the reference's per-head buffer layout (d, K), packed over heads)
 *             embed_t  [H][K][d] fp32, enorm [H][K] fp32 -- derived per step by msmc_vq_prepare
 *   indices   ind      [N][H] int64
 *   diff      diff     [N][d] fp32 (mean over heads of the element-wise squared error)
 */
#ifndef MSMC_HIP_H
#define MSMC_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* msmc_stream;          /* hipStream_t */

#define MSMC_E_SHAPE (-2)           /* unsupported shape (see each function) */
#define MSMC_E_WORKSPACE (-3)       /* workspace too small */

/* Library identity: "gfx950" for the product build, "emu" for the CPU interpreter used by tests. */
const char* msmc_backend(void);
int msmc_abi_version(void);

/* Streams of the library's own (hipStreamNonBlocking), for the side branches of a step: the weight gradients' streams and the
 * resolution discriminators' branch (host side: hip/convnet.py own_streams).  The host framework's stream pool hands the same
 * few streams out again and again; a side stream that IS the stream another part of the step captures on is not a branch.
 * No reference counterpart (the reference runs one stream). */
int msmc_stream_create(msmc_stream* out);
int msmc_stream_destroy(msmc_stream stream);

/* ---------------------------------------------------------------------------------------------
 * V1/V2  multi-head nearest-codeword search with EMA update.
 * Replaces Quantize.forward / MultiHeadQuantize.forward,
 *   reference msmctts/networks/vqgantts/modules.py:24-67 and :137-151.
 * ------------------------------------------------------------------------------------------- */

/* embed [H][d][K] -> embed_t [H][K][d], enorm[h][k] = sum_j embed[h][j][k]^2   (modules.py:29).  d <= 2559 (a tile of 16
 * transposed rows must fit LDS; MSMC_E_SHAPE beyond). */
int msmc_vq_prepare(const float* embed, float* embed_t, float* enorm, int H, int d, int K,
                    msmc_stream stream);

/* Search + gather + straight-through value + head-averaged squared error, all heads, one launch.
 *   dist = (|x|^2 - 2 x.e_k) + |e_k|^2 in fp32, first-minimum tie rule   (modules.py:26-31)
 *   quant[n] = x + (e_best - x) ; diff[n] = (sum_h (e_best - x_h)^2) / H  (modules.py:33,59-60,147)
 * Requires d % 4 == 0 and K % 16 == 0 (MSMC_E_SHAPE otherwise).  Where at least one head's transposed codebook fits LDS
 * (160 KiB) it stays resident; larger codebooks take the streamed kernel below (chunk chosen by the launcher), which
 * additionally needs N * D * 4 < 2^32 and d <= 848.  quant may alias x. */
int msmc_vq_search(const float* x, const float* embed_t, const float* enorm, float* quant, float* diff,
                   int64_t* ind, int N, int D, int H, int K, msmc_stream stream);

/* The same search with no resident codebook (msmc-tts_amd/csrc/vq_stream.inc): every head's codebook passes through LDS
 * in double-buffered chunks of `chunk` codewords while a wave keeps its 16 frames and a running first minimum.  Same
 * distance expression, same fp32 summation order over the d channels, same tie rule: on every shape msmc_vq_search
 * serves with a resident kernel, quant, diff and ind are bit-identical to it.  chunk = 0: the launcher's choice (the
 * largest multiple of 16 that keeps a workgroup at or under 80 KiB of LDS, else under 160 KiB); chunk > 0: forced (a
 * multiple of 16, at most 256; larger than K means K).  Returns MSMC_E_SHAPE for d % 4, K % 16, a chunk that is not a
 * multiple of 16 or does not fit, N * D * 4 >= 2^32; 0 at once for N == 0.  quant may alias x. */
int msmc_vq_search_stream(const float* x, const float* embed_t, const float* enorm, float* quant, float* diff,
                          int64_t* ind, int N, int D, int H, int K, int chunk, msmc_stream stream);

/* Nearest-centroid search of ONE wide head with any number of centroids (msmc-tts_amd/csrc/vq_wide.inc): the k-means unit
 * codebooks of KMeansVQGANEmb (d = 768 / 1024, K = 100 .. 2000), which msmc_vq_search refuses.  Operands as msmc_vq_search
 * with H = 1 (embed_t [K][d] / enorm [K] from msmc_vq_prepare, diff [N][d]); same distance expression and first-minimum
 * tie rule, computed as a GEMM with an arg-min epilogue: frame tiles x centroid tiles, the d axis in double-buffered
 * 32-channel LDS slices, fp32 MFMA.  Takes d % 16 == 0, 16 <= d <= 2048, K >= 1, N >= 0 with N * d * 4 < 2^32
 * (MSMC_E_SHAPE otherwise, nothing launched); 0 at once for N == 0.  quant may alias x. */
int msmc_vq_search_wide(const float* x, const float* embed_t, const float* enorm, float* quant, float* diff,
                        int64_t* ind, int N, int d, int K, msmc_stream stream);

/* The labels of that search and nothing else (msmc-tts_amd/csrc/vq_assign.inc): unit extraction over a corpus wants 8 bytes
 * per frame, not quant and diff.  Operands as msmc_vq_search_wide; the search is the same code in the same instantiation
 * (msmc_vq_wide_set_split included), so ind [N] is what msmc_vq_search_wide writes for these inputs, bit for bit (first
 * minimum on ties).  dist [N] (may be NULL: then only ind is written) is the squared distance to the winner's row e =
 * embed_t[ind[n]], recomputed as direct fp32 differences -- 0 exactly for a frame that equals its centroid, never the
 * expanded form -- in a fixed order that does not depend on the split: the 16-byte pieces c4 = 0 .. d / 4 - 1 of the row go to
 * 16 partial sums, piece c4 to partial c4 % 16; partial[p] = (((+0 + s_0) + s_1) + ...) over (x - e)^2 of the pieces p, p + 16,
 * ... in ascending order and of the four channels of a piece in order; dist[n] = (((+0 + partial[0]) + partial[1]) + ... +
 * partial[15]).  One rounding per difference, product and add.  No atomics.
 * Takes d % 16 == 0, 16 <= d <= 2048, K >= 1, N >= 0 with N * d * 4 < 2^32, x and embed_t 16-byte aligned (MSMC_E_SHAPE
 * otherwise, nothing launched); 0 at once for N == 0. */
int msmc_vq_assign_wide(const float* x, const float* embed_t, const float* enorm, int64_t* ind, float* dist, int N, int d,
                        int K, msmc_stream stream);

/* The same search -- identical indices, quant and diff, bit for bit -- under the HBM roof for K >= 64
 * (msmc-tts_amd/csrc/vq_shortlist.inc): all K distances approximately on the bf16 matrix cores (two-piece bf16 splits of
 * x and e, three products), a running top-2 per frame, and a rigorous error bound that decides per (frame, head) whether
 * the approximate winner IS the exact kernel's first minimum; where it is not (near-ties, duplicate codewords) the
 * 16-frame tile is searched again with the exact fp32 chain.  The codebook comes as a prepared image
 * (msmc_vq_prepare_shortlist, from embed_t / enorm of msmc_vq_prepare; msmc_vq_shortlist_bytes = its size, 0 when the
 * kernel does not take the shape: d = D/H in {32, 64}, K % 16 == 0, one head's image <= 78 KiB).  slow_count (may be NULL):
 * two counters, incremented once per 16-frame tile and head that took [0] the exact re-rank of the best two candidates,
 * [1] the exact re-search over all K.  Finite inputs; magnitudes above bf16 underflow. */
size_t msmc_vq_shortlist_bytes(int H, int d, int K);
int msmc_vq_prepare_shortlist(const float* embed_t, const float* enorm, void* image, int H, int d, int K,
                              msmc_stream stream);
int msmc_vq_search_shortlist(const float* x, const float* embed_t, const float* enorm, const void* image, float* quant,
                             float* diff, int64_t* ind, unsigned long long* slow_count, int N, int D, int H, int K,
                             msmc_stream stream);

/* Bytes of scratch msmc_vq_ema_update needs for these sizes. */
size_t msmc_vq_ema_workspace(int N, int D, int H, int K);

/* EMA statistics over the valid frames (t < length[b]) followed by the in-place buffer update
 *   cluster_size <- decay*cluster_size + (1-decay)*count ; embed_avg <- decay*embed_avg + (1-decay)*sum
 *   embed <- embed_avg / ((cluster_size+eps)/(n+K*eps)*n)                     (modules.py:35-57)
 * Deterministic: per-tile partial sums are reduced in a fixed order.
 * x [B*T][D], ind [B*T][H], length [B] int64. */
int msmc_vq_ema_update(const float* x, const int64_t* ind, const int64_t* length, float* embed,
                       float* cluster_size, float* embed_avg, void* workspace, size_t workspace_bytes,
                       int B, int T, int D, int H, int K, float decay, float eps, msmc_stream stream);

/* The two halves of msmc_vq_ema_update, for data-parallel codebook synchronisation (an option the reference does not
 * have: its ranks EMA-update from their local batch, distributed.py:154-204 never touches buffers): _stats writes
 * stats = [H][K][d] per-codeword sums followed by [H][K] counts of THIS rank's valid frames; the host sums `stats` over
 * ranks (one all-reduce) and _apply performs the buffer update from the summed statistics.  _stats + _apply on one rank
 * is bit-identical to msmc_vq_ema_update.  stats: H*K*(D/H + 2) floats (sums, counts, H*K of scratch for _apply). */
int msmc_vq_ema_stats(const float* x, const int64_t* ind, const int64_t* length, float* stats, void* workspace,
                      size_t workspace_bytes, int B, int T, int D, int H, int K, msmc_stream stream);
int msmc_vq_ema_apply(float* stats, float* embed, float* cluster_size, float* embed_avg, int D, int H, int K,
                      float decay, float eps, msmc_stream stream);

/* The same update for ONE wide head, beyond d = 512 (msmc-tts_amd/csrc/ema_wide.hip): the shapes of msmc_vq_search_wide,
 * d % 16 == 0, 16 <= d <= 2048, K >= 1, with N = B*T >= 1, N * d * 4 < 2^32 and x / stats / workspace 16-byte aligned;
 * anything else returns MSMC_E_SHAPE with nothing launched and nothing written.  x [B*T][d], ind [B*T], length [B] int64,
 * embed / embed_avg [d][K], cluster_size [K].  Frames with t >= length[b] are never read.
 * _workspace: bytes of scratch of _update: 8 N rounded up to 16 for the masked labels, msmc_kmeans_stats_workspace(N, d, K), and
 * 4 K (d + 2) for a stats block; 0 for a refused shape.  _stats needs the first two parts only.  A shorter workspace:
 * MSMC_E_WORKSPACE.
 * _stats: lab[n] = ind[n] where t < length[b] (n = b*T + t), else -1, then the launches of msmc_kmeans_stats on (x, lab): stats =
 * [K][d] sums, [K] counts, K floats of scratch for _apply -- the layout of msmc_vq_ema_stats with H = 1.  _apply: the buffer
 * update from stats (summed over ranks where the host does that).  _update: _stats into the workspace's stats block, then
 * _apply; bit-identical to calling the two.
 * Fixed order of every operation (same inputs, same bits; no floating-point atomics): the sums in the run order of
 * msmc_kmeans_stats (below); omd = (float)(1.0 - (double)decay), keps = (float)((double)K * (double)eps);
 * cs_new[k] = fmaf(counts[k], omd, cluster_size[k] * decay); n = the sum of cs_new as msmc_vq_ema_update forms it: 256 partials
 * p[t] = ((+0 + cs_new[t]) + cs_new[t + 256]) + ..., then p[t] = p[t] + p[t + s] for t < s, s = 128, 64, .. 1, n = p[0];
 * sm[k] = (cs_new[k] + eps) / (n + keps) * n, left to right; embed_avg[j][k] = fmaf(sums[k][j], omd, embed_avg[j][k] * decay);
 * embed[j][k] = embed_avg[j][k] / sm[k]; cluster_size[k] = cs_new[k].  Every operation named is one IEEE fp32 operation.
 * On a shape msmc_vq_ema_update takes as well, counts and cluster_size are bit-identical to it; embed and embed_avg differ by the
 * summation order of the sums alone. */
size_t msmc_vq_ema_wide_workspace(int N, int d, int K);
int msmc_vq_ema_wide_stats(const float* x, const int64_t* ind, const int64_t* length, float* stats, void* workspace,
                           size_t workspace_bytes, int B, int T, int d, int K, msmc_stream stream);
int msmc_vq_ema_wide_apply(float* stats, float* embed, float* cluster_size, float* embed_avg, int d, int K, float decay,
                           float eps, msmc_stream stream);
int msmc_vq_ema_wide_update(const float* x, const int64_t* ind, const int64_t* length, float* embed, float* cluster_size,
                            float* embed_avg, void* workspace, size_t workspace_bytes, int B, int T, int d, int K, float decay,
                            float eps, msmc_stream stream);

/* Backward of (quant, diff) wrt x:  gx = g_quant + g_diff * 2*(x - quant)/H   (straight-through +
 * the un-reduced commitment term, modules.py:59-60).  g_diff may be NULL (treated as zero). */
int msmc_vq_backward(const float* g_quant, const float* g_diff, const float* x, const float* quant,
                     float* gx, int N, int D, int H, msmc_stream stream);

/* ---------------------------------------------------------------------------------------------
 * KM  the M step of Lloyd's algorithm for the k-means unit codebooks of KMeansVQGANEmb (msmc-tts_amd/csrc/kmeans.hip;
 * the E step is msmc_vq_prepare + msmc_vq_search_wide; the loop is msmctts_amd/hip/kmeans.py fit_kmeans).
 * No reference counterpart: the reference loads a k-means model fitted elsewhere (msmc_vqgan_emb.py:294-336).
 * ------------------------------------------------------------------------------------------- */

/* Bytes of scratch msmc_kmeans_stats needs for these sizes: 4 (P K + 2 (K + 1) + N) rounded up to 16, with P <= 256 parts
 * and P K <= N + K, plus 4 d (N / 64 + min(K, N)) for the run partials.  0 for N <= 0 or a shape the kernel refuses. */
size_t msmc_kmeans_stats_workspace(int N, int d, int K);

/* Per-centroid sums and counts of labelled frames: x [N][d], ind [N] -> sums [K][d], counts [K] (fp32; exact below 2^24
 * rows per centroid).  sums[k] = sum of the rows n with ind[n] == k, counts[k] = their number; entries of ind outside
 * [0, K) are skipped (the mask for padding).  accumulate = 0 overwrites sums / counts, accumulate = 1 adds this call's
 * totals onto what they hold, one add per element (blocks of frames folded in a fixed order).
 * Deterministic, no floating-point atomics.  Summation order, per channel: the rows of centroid k in ascending n are cut
 * into runs of 64 rows; a run partial is (((+0 + x[n_0]) + x[n_1]) + ...) over its rows in ascending n; the centroid's
 * total is (((+0 + partial_0) + partial_1) + ...) over its runs in ascending order; sums[k] = total, or sums[k] + total with
 * accumulate.  An empty centroid has total +0 and count 0.
 * Takes d % 4 == 0, 4 <= d <= 2048, K >= 1, N >= 0, N * d * 4 < 2^32 and x, sums, workspace 16-byte aligned: MSMC_E_SHAPE
 * otherwise, nothing launched.  MSMC_E_WORKSPACE for a workspace below msmc_kmeans_stats_workspace.  N == 0: returns 0 and,
 * without accumulate, writes zeros (no workspace needed). */
int msmc_kmeans_stats(const float* x, const int64_t* ind, float* sums, float* counts, void* workspace, size_t workspace_bytes,
                      int N, int d, int K, int accumulate, msmc_stream stream);

/* Centre update, in place: centers[k][c] = sums[k][c] / counts[k] (IEEE fp32 division) where counts[k] > 0; an empty
 * centroid keeps its row.  shift2[k] = squared movement of row k (+0 for an empty centroid), summed in a fixed order: lane l
 * of a 64-lane wave adds (new - old)^2 of the 4-channel pieces l, l + 64, l + 128, ... in ascending channel order from +0,
 * then the 64 lane sums are added as a butterfly, v = v + v[lane ^ m] for m = 1, 2, 4, 8, 16, 32.
 * Takes d % 4 == 0, 4 <= d <= 2048, K >= 1, sums / centers 16-byte aligned (MSMC_E_SHAPE otherwise). */
int msmc_kmeans_update(const float* sums, const float* counts, float* centers, float* shift2, int d, int K,
                       msmc_stream stream);

/* Bytes of scratch msmc_kmeanspp_seed needs: 128 of state, float64 prefixes 8 L (T + 1) and tile partials 8 L T (each rounded
 * up to 16) with T = ceil(N / 256) tiles, and two buffers of minima 4 L N (each rounded up to 16).  0 for a shape the
 * kernels refuse. */
size_t msmc_kmeanspp_workspace(int N, int d, int K, int L);

/* Greedy k-means++ seeding (msmc-tts_amd/csrc/kmeans_pp.hip): K frames of x [N][d] as the first centres of Lloyd's
 * algorithm.  centre 0 = x[first], mind[n] = |x[n] - centre 0|^2; step i = 1 .. K - 1 draws L candidates, candidate j = the
 * first frame n with cum[n] > u[i - 1][j] * total (cum: the running sum of mind, total its last value; u [K - 1][L] float64 in
 * [0, 1)), evaluates pot[j] = sum over n of min(mind[n], |x[n] - x[candidate j]|^2) for all of them in ONE pass over x, and
 * keeps the candidate of the smallest pot (ties: the lowest j): its row is centre i, mind takes the minimum with its distances.
 * Outputs: centers [K][d] (the chosen rows), chosen [K] (their frame numbers), potential [K] (the sum of mind after every
 * pick).  Enqueues everything -- two launches per centre -- on the stream: no read-back, no allocation.
 * Fixed order of every sum (same inputs, same bits): distances in fp32 as the direct difference, per frame in the order of
 * shift2 above; cum, total and pot in float64: within a tile of 256 frames local[n] = ((+0 + m[n0]) + ...) + m[n] in
 * ascending n, pre[t + 1] = pre[t] + local[last frame of tile t] over the tiles in ascending order from +0, cum[n] =
 * pre[t] + local[n], total = pot = pre[T].  cum never decreases and ends at total bit for bit; a frame of weight 0 is never
 * picked; total == 0 (every frame coincides with a centre, e.g. K > N) picks frame N - 1: duplicate centres.
 * Takes d % 4 == 0, 4 <= d <= 2048, K >= 1, 1 <= L <= 16, 1 <= N < 2^31, 0 <= first < N, x / centers / workspace 16-byte
 * aligned (rows are addressed with 64-bit offsets: N d 4 may exceed 2^32): MSMC_E_SHAPE otherwise, nothing launched.
 * MSMC_E_WORKSPACE for a workspace below msmc_kmeanspp_workspace. */
int msmc_kmeanspp_seed(const float* x, int N, int d, int K, int L, long first, const double* u, float* centers, int64_t* chosen,
                       double* potential, void* workspace, size_t workspace_bytes, msmc_stream stream);

/* ---------------------------------------------------------------------------------------------
 * UN  from labels to units (msmc-tts_amd/csrc/units.hip; the labels: msmc_vq_assign_wide; host side msmctts_amd/hip/units.py).
 * The reference counts code usage on the host with a dictionary (examples/qs-tts/scripts/vq_analysis.py
 * compute_codebook_complexity) and has no run collapse.  Integer work: both results are exact.
 * ------------------------------------------------------------------------------------------- */

/* Run-length collapse of the valid prefix ind[b][0 .. min(length[b], T)) of every utterance, ind [B][T], length [B]: maximal
 * runs of equal labels, run r -> units[b][r] (the label), dur[b][r] (its frames), ulen[b] = the number of runs; the slots
 * r >= ulen[b] get units = -1 and dur = 0.  units [B][T], dur [B][T], ulen [B]: every element is written exactly once, nothing
 * at or beyond length[b] is read, length[b] <= 0 gives ulen[b] = 0.  One workgroup per utterance, any T.
 * B <= 0 or T <= 0: MSMC_E_SHAPE. */
int msmc_units_collapse(const int64_t* ind, const int64_t* length, int64_t* units, int32_t* dur, int64_t* ulen, int B, int T,
                        msmc_stream stream);

/* counts[k] = the number of valid frames (t < min(length[b], T)) of ind [B][T] labelled k, counts [K] int64; labels outside
 * [0, K) are skipped.  accumulate = 0 overwrites counts, accumulate = 1 adds onto what it holds (a corpus, batch by batch).
 * Integer adds only (LDS counters per workgroup, then 64-bit adds in global memory): exact in any order.
 * B <= 0, T <= 0 or K <= 0: MSMC_E_SHAPE. */
int msmc_units_usage(const int64_t* ind, const int64_t* length, int64_t* counts, int B, int T, int K, int accumulate,
                     msmc_stream stream);

/* total[b] = the int64 sum of max(dur[b][r], 0) over r < min(max(ulen[b], 0), R): the frames msmc_units_expand makes of
 * utterance b when T does not cut them.  dur [B][R] int32, ulen [B] int64, total [B] int64.  Nothing at or beyond ulen[b] is
 * read.  B <= 0 or R <= 0: MSMC_E_SHAPE. */
int msmc_units_total(const int32_t* dur, const int64_t* ulen, int64_t* total, int B, int R, msmc_stream stream);

/* The inverse of msmc_units_collapse: units [B][R] int64, dur [B][R] int32, ulen [B] int64 -> ind [B][T] int64, length [B]
 * int64.  Run r < min(max(ulen[b], 0), R) of utterance b covers the frames [s_r, s_r + max(dur[b][r], 0)), s_r = the sum of
 * max(dur, 0) over the runs before it, in 64 bits; total = that sum over all runs.  ind[b][t] = units[b][r] of the run that
 * covers t for t < min(total, T), -1 from there on; length[b] = min(total, T).  Runs of zero or negative duration make no
 * frame.  Every element of ind and length is written exactly once; nothing at or beyond ulen[b] is read.  One workgroup per
 * utterance, 256 runs at a time, any R and T; consecutive work-items write consecutive frames.
 * B <= 0, R <= 0 or T <= 0: MSMC_E_SHAPE, nothing launched. */
int msmc_units_expand(const int64_t* units, const int32_t* dur, const int64_t* ulen, int64_t* ind, int64_t* length, int B, int R,
                      int T, msmc_stream stream);

/* ---------------------------------------------------------------------------------------------
 * UE  the decoder input of KMeansVQGANEmb from unit labels (msmc-tts_amd/csrc/unit_embed.hip; host side msmctts_amd/hip/units.py
 * unit_embed).  The reference embeds the labels, runs the nearest-centroid search on the result and then in_linear
 * (msmc_vqgan_emb.py:440-446); with a frozen codebook that is a row of table = centers W^T + b [K][C].
 * A row (b, t) is VALID when t < length[b] and 0 <= ind[b][t] < K.  ind [B][T] int64, length [B] int64, fp32 elsewhere.
 * Shapes: C % 8 == 0, 8 <= C <= 2048, K >= 1, B >= 1, T >= 1, every fp32 pointer (and the workspace) 16-byte aligned; the
 * backward also needs B T C 4 < 2^32.  Anything else: MSMC_E_SHAPE, nothing launched, nothing written.
 * ------------------------------------------------------------------------------------------- */

/* out[b][t][:] = table[ind[b][t]][:] + glob[b][:] on the valid rows -- one fp32 add per element, none when glob is NULL (then
 * the row is the table's, bit for bit) -- and +0 in every other row.  table [K][C], glob [B][C] or NULL, out [B][T][C].  The
 * table is never read at an invalid label; every element of out is written exactly once (16-byte loads and stores). */
int msmc_units_embed_fwd(const int64_t* ind, const int64_t* length, const float* table, const float* glob, float* out, int B, int T,
                         int C, int K, msmc_stream stream);

/* Bytes of scratch that are enough for msmc_units_embed_bwd on N = B T frames whatever B is: two int64 label arrays 8 N (each
 * rounded up to 16), 4 max(K, N) of counts (rounded up to 16) and the larger of msmc_kmeans_stats_workspace(N, C, K) and
 * (N, C, N).  0 for a refused shape.  (A call needs the same with its own B in the place of N, which is never more.) */
size_t msmc_units_embed_workspace(int N, int C, int K);

/* The gradient of msmc_units_embed_fwd: gtable[k] = the sum of gout[n] over the valid rows labelled k, gglob[b] = the sum of
 * gout[b][t] over the valid rows of utterance b (skipped when gglob is NULL).  gout [B][T][C], gtable [K][C], gglob [B][C]:
 * both are overwritten, not accumulated; rows without a valid frame come out +0.
 * Fixed order (same inputs, same bits; no floating-point atomics): lab[n] = ind[n] on the valid rows, -1 elsewhere, and the
 * launches of msmc_kmeans_stats on (gout, lab) with K labels; ulab[n] = b on the valid rows, -1 elsewhere, and the same launches
 * on (gout, ulab) with B labels.  So, per channel: the rows of a label (of an utterance) in ascending n (t) are cut into runs of
 * 64; a run partial is (((+0 + g[n_0]) + g[n_1]) + ...), the total (((+0 + partial_0) + partial_1) + ...).
 * MSMC_E_WORKSPACE for a workspace shorter than the call needs (see msmc_units_embed_workspace). */
int msmc_units_embed_bwd(const float* gout, const int64_t* ind, const int64_t* length, float* gtable, float* gglob, void* workspace,
                         size_t workspace_bytes, int B, int T, int C, int K, msmc_stream stream);

/* ---------------------------------------------------------------------------------------------
 * SE  the pitch / energy side encoder of MAMSEncoder (msmc-tts_amd/csrc/side_enc.hip; host side msmctts_amd/hip/side_enc.py
 * side_front / pool_add).  Replaces, reference msmctts/networks/vqgantts/msmc_vqgan_emb.py:61-66 and :95-112, the torch.cat of
 * the two tracks, the first Conv1d (P + E input channels: below the 8-channel granularity of the convolution kernels) with its
 * Tanh, and per stage the transposes around avg_pool1d(ceil_mode=True) of the side encoding and the addition to the stage output.
 * All tensors channels-last and contiguous.  Every sum runs in a fixed order (source header): no floating-point atomics, same
 * inputs, same bits within one build.  A refused shape returns MSMC_E_SHAPE; nothing is launched, nothing written.
 * ------------------------------------------------------------------------------------------- */

/* y [B][T][C] (y_dtype 0 = fp32, 1 = bf16; 16-byte aligned) = tanhf(bias[c] + sum_ci sum_k w[c][ci][k] x[b][t + k - (taps-1)/2][ci]),
 * x = 0 outside [0, T); input channel ci < P is pitch [B][T][P], the others energy [B][T][E] (fp32; a pointer may be NULL where
 * its width is 0).  w [C][P + E][taps], bias [C]: nn.Conv1d's layout, fp32, accumulated in fp32.  No length masking.  One launch.
 * Takes 1 <= P + E <= 8, taps odd and <= 15, C % 8 == 0, C (P + E) taps + C <= 12288 (the weight is staged in LDS). */
int msmc_side_front_fwd(const float* pitch, const float* energy, const float* w, const float* bias, void* y, int y_dtype, int B, int T,
                        int P, int E, int C, int taps, msmc_stream stream);

/* Bytes of the backward's scratch: one set of (dw, db) partials per tile of 32 frames of an utterance; 0 for a refused shape. */
size_t msmc_side_front_bwd_workspace(int B, int T, int P, int E, int C, int taps);

/* dw [C][P + E][taps] and db [C] (fp32, overwritten) from y and gy [B][T][C] (both y_dtype): dz = gy (1 - y y) in fp32,
 * dw = sum_{b,t} dz x, db = sum_{b,t} dz.  Two launches: per-tile partials, then their sum in ascending tile order.  No gradient
 * to pitch / energy.  workspace 16-byte aligned, at least msmc_side_front_bwd_workspace bytes: MSMC_E_WORKSPACE otherwise. */
int msmc_side_front_bwd(const float* pitch, const float* energy, const void* y, const void* gy, int y_dtype, float* dw, float* db,
                        void* workspace, size_t workspace_bytes, int B, int T, int P, int E, int C, int taps, msmc_stream stream);

/* side [B][Tin][C] fp32, feat [B][Tout][C] (feat_dtype 0 = fp32, 1 = bf16), Tout == ceil(Tin / scale), scale >= 1:
 * pooled [B][Tout][C] fp32 = the mean of the in-bounds frames of window u (summed in ascending frame, divided by their count:
 * avg_pool1d(kernel = stride = scale, ceil_mode = True, padding = 0)); out [B][Tout][C] in feat's dtype = feat + cast(pooled).
 * scale == 1: out = feat + cast(side); pooled is not touched and may be NULL.  One launch. */
int msmc_pool_add_fwd(const float* side, const void* feat, int feat_dtype, float* pooled, void* out, int B, int Tin, int Tout, int C,
                      int scale, msmc_stream stream);

/* gside [B][Tin][C] fp32 = (gout + gpooled)[b][t / scale][c] / (frames of that window); gout [B][Tout][C] in gout_dtype, gpooled
 * [B][Tout][C] fp32; either may be NULL (not both).  Every element of gside is written once.  One launch.  (The gradient of
 * feat is gout itself.) */
int msmc_pool_add_bwd(const void* gout, int gout_dtype, const float* gpooled, float* gside, int B, int Tin, int Tout, int C, int scale,
                      msmc_stream stream);

/* ---------------------------------------------------------------------------------------------
 * UC  the unit predictor's loss and label decoding (msmc-tts_amd/csrc/unit_ce.hip; host side msmctts_amd/hip/unit_ce.py
 * masked_cross_entropy / unit_argmax).  Replaces the 'softmax' chain of MultiStageQuantizer.compute_embedding_loss, reference
 * msmctts/networks/vqgantts/msmc_vqgan.py:254-258 with the masking of :266-268 -- cross_entropy(reduction='none'), masked_fill,
 * sum, / sum of lengths -- which stores [N][K] fp32 log-probabilities and cannot take the -1 padding of unit labels.
 * logits [B][T][ld], dtype 0 = fp32, 1 = bf16: the first K columns of a row are the classes, 1 <= K <= ld (ld: the width of a
 * projection built wider than K).  target [B][T] int64; lengths [B] int32 (len_is_64 = 0) or int64.  Row (b, t) is VALID when
 * t < lengths[b]; the logits of other rows are never read.  A valid row whose target is outside [0, K) is IGNORED: no loss, zero
 * gradient.  The denominator is the sum of the lengths as given.  A wave per row, any K; 16-byte loads and stores where
 * ld % (4 fp32 / 8 bf16) == 0 and logits (and glogits) are 16-byte aligned, element accesses otherwise -- the two paths add in
 * different orders (both documented in the source's header) and may differ in the last bits.
 * K < 1, K > ld, B < 1, T < 1, B T >= 2^31, another dtype or a NULL operand: MSMC_E_SHAPE, nothing launched, nothing written.
 * ------------------------------------------------------------------------------------------- */

/* Bytes of the forward's scratch (one fp32 partial and one int count per workgroup, each array rounded up to 16 bytes); 0 for a
 * refused B, T. */
size_t msmc_unit_ce_workspace(int B, int T);

/* Two launches.  lse [B][T] fp32 = m + logf(sum_k expf(x_k - m)), m the row maximum, on valid rows (0 elsewhere); pred [B][T]
 * int64 (may be NULL) = the arg-max over the K classes, lowest index on ties (exact: comparisons only), -1 on padded rows;
 * out[0] = (sum over valid, not ignored rows of lse - x[target]) / sum of lengths, out[1] = 1 / sum of lengths (for the backward
 * pass); correct (int64[1], may be NULL) = the rows with pred == target.  sum of lengths <= 0: out[0] = out[1] = 0.
 * Every sum runs in a fixed order (source header), no floating-point atomics: same inputs, same bits within one build.
 * workspace 16-byte aligned, at least msmc_unit_ce_workspace(B, T) bytes: MSMC_E_WORKSPACE otherwise, nothing launched. */
int msmc_unit_ce_fwd(const void* logits, int dtype, const int64_t* target, const void* lengths, int len_is_64, float* lse, int64_t* pred,
                     float* out, int64_t* correct, void* workspace, size_t workspace_bytes, int B, int T, int K, int ld,
                     msmc_stream stream);

/* One launch.  glogits [B][T][ld] in the logits' dtype = (expf(x_k - lse) - [k == target]) * gout[0] * out[1] for k < K on valid,
 * not ignored rows; +0 in the columns K .. ld - 1, on padded rows and on ignored rows.  Every element is written exactly once. */
int msmc_unit_ce_bwd(const void* logits, int dtype, const int64_t* target, const void* lengths, int len_is_64, const float* lse,
                     const float* out, const float* gout, void* glogits, int B, int T, int K, int ld, msmc_stream stream);

/* The forward's arg-max alone (the same device function: the same labels): pred [B][T] int64, -1 on padded rows.  One launch. */
int msmc_unit_argmax(const void* logits, int dtype, const void* lengths, int len_is_64, int64_t* pred, int B, int T, int K, int ld,
                     msmc_stream stream);

/* ---------------------------------------------------------------------------------------------
 * CE  stage targets of the multi-stage quantiser from stored code indices (msmc-tts_amd/csrc/code_embed.hip; host side
 * msmctts_amd/hip/code_embed.py code_gather; MultiStageQuantizer.embed_codes).  With a frozen codebook the quantised output of a
 * stage is, head by head, a codebook row: this replaces, for a predictor step on stored codes, the frozen autoencoder's whole
 * analysis (reference msmctts/trainers/emb_vqgan_trainer.py:202-210).  Forward only.
 * ------------------------------------------------------------------------------------------- */

/* out[b][t][h d + c] = embed_t[h][ind[b][t][h]][c] where t < length[b] and 0 <= ind[b][t][h] < K; the d channels of a head
 * whose label is outside [0, K) are +0 (nothing is read for that head), and so is every row t >= length[b].
 * ind [B][T][H] int32 (ind_i64 = 0) or int64 (1); length [B] int32 on the device (any value: <= 0 makes the utterance all
 * zeros); embed_t [H][K][d] fp32, the layout msmc_vq_prepare writes; out [B][T][H d] fp32 (out_bf16 = 0) or bf16 (1: one
 * rounding to nearest even).  One launch; every element of out is written exactly once with plain stores (no zero-fill, no
 * atomics); a label is range-checked before it forms an address.  d % 4 == 0 with embed_t and out 16-byte aligned: 16-byte
 * loads and stores (bf16 out: one 16-byte store per 8 channels where d % 8 == 0, else 8 bytes per 4 channels); any other d >= 1
 * or alignment: one element per access, the same values.
 * B < 1, T < 1, H < 1, d < 1, K < 1, a flag outside {0, 1}, a NULL operand or a row of 2^31 - 2048 pieces or more:
 * MSMC_E_SHAPE, nothing launched, nothing written.  The caller guarantees the shapes above (contiguous). */
int msmc_code_gather(const void* ind, int ind_i64, const int* length, const float* embed_t, void* out, int out_bf16,
                     int B, int T, int H, int d, int K, msmc_stream stream);

/* ---------------------------------------------------------------------------------------------
 * G1/G2/D1/D2 channels-last implicit-GEMM convolution family on the matrix cores.
 * Replaces the cuDNN/MIOpen convolutions behind
 *   Generator.forward / ResBlock1.forward   reference msmctts/networks/hifigan/generator.py:40-55, common.py:44-51
 *   DiscriminatorP.forward                  reference msmctts/networks/hifigan/discriminator.py:135-154
 *   DiscriminatorR.forward                  reference msmctts/networks/hifigan/discriminator.py:71-76
 * One "gather" kernel serves forward convolutions (dilated / strided / reflect- or zero-padded),
 * transposed convolutions and every data-gradient (as per-phase sub-lattices); one kernel computes
 * weight gradients.  Activations are channels-last [B][H][W][C] (1-D signals: H = 1); dtype 0 = fp32
 * (exact-fp32 MFMA), 1 = bf16 storage with fp32 accumulation.
 * ------------------------------------------------------------------------------------------- */
#define MSMC_CONV_MAX_TAPS 16

typedef struct msmc_conv_desc {
    const void* x;          /* input  [B][Hin][Win][Cin]                                                  */
    const void* w;          /* weight slices [nslice][Cout][Cin], same dtype as x                          */
    const float* bias;      /* [Cout] fp32 or NULL                                                         */
    const void* mask_src;   /* NULL, or [B][Hout][Wout][Cout]: v *= (mask_src > 0 ? 1 : mask_slope)        */
    const void* res;        /* NULL, or [B][Hout][Wout][Cout]: v = v + res                                 */
    const void* res2;       /* NULL, or same shape: v = res2 + v                                           */
    void* out;              /* [B][Hout][Wout][Cout]                                                       */
    int dtype;              /* 0 fp32, 1 bf16                                                              */
    int B, Hin, Win, Cin, Hout, Wout, Cout;
    /* output sub-lattice: (oy, ox) = (oy0 + qy*osy, ox0 + qx*osx), qy < QH, qx < QW                       */
    int QH, QW, oy0, osy, ox0, osx;
    /* input coordinate of tap t at lattice point q: (qy*isy + iy0 + tap_dy[t], qx*isx + ix0 + tap_dx[t])  */
    int isy, isx, iy0, ix0;
    int ntaps;
    int tap_dy[MSMC_CONV_MAX_TAPS], tap_dx[MSMC_CONV_MAX_TAPS], tap_w[MSMC_CONV_MAX_TAPS];
    int pad_mode;           /* 0 = zeros outside the input, 1 = reflect                                    */
    float in_slope;         /* leaky-ReLU slope applied to x on load (1 = identity)                        */
    float mask_slope;
    float out_div;          /* v = v / out_div when != 1                                                   */
    float out_slope;        /* leaky-ReLU slope applied to v last (1 = identity)                           */
    int variant;            /* kernel choice, 0 = library heuristic.  msmc_conv_gather: 1 = first-generation dispatch
                               (pipelined / simple kernel), 2 = second generation with 128-byte channel chunks where
                               they fit, 3 = second generation, 64-byte chunks, 4 / 5 = as 2 / 3 with eight instead of
                               four weight vectors in flight per work-item, 6 / 7 = as 2 / 3 with the whole channel chunk in flight
                               and the next chunk prefetched (small grids; MSMC_E_SHAPE when the chunk exceeds 16 vectors
                               per work-item), 8 = direct (matrix-core-free) kernels for <= 8 -> <= 16 channel layers,
                               C -> 1 and 1 -> C layers (MSMC_E_SHAPE otherwise), 16..23 = third generation (bf16: 64-row wave
                               tiles, LDS-DMA weight stream, one barrier per chunk; 16 + (256- instead of 128-point tiles) +
                               2*(64- instead of 32-column wave tiles) + 4*(128- instead of 64-byte chunks); MSMC_E_SHAPE
                               where a configuration does not apply), 24..31 = 16..23 with the halo tile by LDS-DMA as well (no staging
                               registers; unpadded source-swizzled rows, zero chunk for padding pixels, in-place input activation,
                               0 <= in_slope <= 1), 32 = persistent thin-layer kernel (csrc/gather4.inc: Cin, Cout in {32, 64}, unit strides, zero
                               padding, taps along one axis; weights of all taps resident in LDS, halo tiles by LDS-DMA, epilogue in
                               registers; MSMC_E_SHAPE outside that scope), 33 = 32 with the epilogue of a tile deferred into the next
                               iteration (measured no faster: not a tuner candidate), 34 = 1-tap unit-stride layers as a plain channel GEMM
                               (csrc/gemm1.inc: 128 x 128 tiles, both operands by LDS-DMA in 64-channel chunks, epilogue in
                               registers; bf16 with Cin % 8 == 0, or exact fp32 -- v_mfma_f32_32x32x2_f32, fp32 output -- with Cin % 4 == 0;
                               Cout % 4 == 0; MSMC_E_SHAPE for anything but a kernel-size-1 layer on the identity lattice), 35 = 34 with
                               64 x 128 tiles on eight waves (GEMMs with few pixel rows), 36 / 37 = 34 / 35 for fp32 data times a CONSTANT matrix
                               given as its pre-split bf16 image (w: [Cout][ceil(Cin / 32)][hi 32 | lo 32] bf16, hi = bf16(w), lo = bf16(w - hi);
                               three products w_hi x_hi + w_lo x_hi + w_hi x_lo on v_mfma_f32_32x32x16_bf16 with fp32 accumulation and fp32
                               output, ~2^-16 relative; no epilogue operands: the framed-DFT / mel GEMMs of the bf16 configuration), 40..46 = fifth generation (csrc/gather5.inc, bf16,
                               >= 2 taps, Cin % 64 == 0, Cout % 8 == 0: sixteen waves, stages of (64-channel chunk, tap) with the weight
                               slices in an LDS-DMA ring and the halo tile of a chunk shared by its taps, epilogue in registers with 16-byte
                               stores; tiles 40: 128 x 128, 41: 256 x 128, 42 / 43: 128 x 256, 44: 64 x 256, 45: 64 x 128 with the
                               contraction split over two groups of eight waves (Cin % 128 == 0), 46: 256 x 64, 47: 128 x 128 for one-chunk layers
                               with halo tiles of up to 640 pixels; MSMC_E_SHAPE where a configuration does not apply), 50 = thin-channel
                               kernel (csrc/gather6.inc: Cin in {2, 4, 8, 16, 32, 64}, Cout <= 64, Cin * taps <= 704; B fragments loaded
                               straight from global memory, weights in LDS, no workgroup barriers in the tile loop), 9 = 32-point tiles with the channel
                               chunks split over the four waves (deep reductions on small grids).  msmc_conv_wgrad (bf16): 1 = first,
                               2 = second generation (fp32 atomics), 3 = third (split partials + fixed-order reduce), 4 / 5 / 6 = fourth (the
                               third's result contract; pixel tiles flow through an LDS-DMA ring: 4 = three stages, fragment reads two
                               steps ahead of the MFMAs, 5 = one step ahead, 6 = two stages, one step ahead;
                               MSMC_E_SHAPE outside its scope: unit strides, zero padding, channel counts multiples of 64,
                               taps along one axis), 7 = the third generation's lattice tiles with both operands staged by LDS-DMA into
                               a two-stage ring (csrc/wgrad5.inc: strided, 2-D and reflection-padded layers with channel counts that
                               are multiples of 64; a tuner candidate since round 3), 8 = direct kernel for thin layers (csrc/wgrad6.inc:
                               one lattice point per work-item, a block of <= 128 elements of dW in registers, atomics into the
                               privatised copies as generations 1 / 2; MSMC_E_SHAPE when dW needs more than 96 such blocks).  The host
                               layer times the candidates once per layer shape.       */
    int split_shift;        /* msmc_conv_wgrad: pixel split = model << split_shift (>> when negative).  msmc_conv_gather
                               variants 16..31 and 40..46 only: DIAGNOSTICS mask, 0 in production (1 skip the MFMAs, 2 the weight stream,
                               4 the halo loads, 8 the epilogue: tools/bench_gather3.py ABLATE=...; results are then garbage) */
    int dw_copies;          /* msmc_conv_wgrad: R > 1 = dw is [R][ntaps][Cout][Cin] and db [R][Cout]; workgroup i adds
                               into copy i % R (same-address atomics retire serially; R copies shorten the chain R
                               times); the consumer sums the copies (msmc_wn_backward_multi does)                      */
} msmc_conv_desc;

/* ---------------------------------------------------------------------------------------------
 * Attention core of the FFT blocks (bf16; fp32: the _f32 pair below; head size 64): softmax(q k^T * scale + bias) (dropout) v per (batch, head),
 * q / k / v read in place from the fused projection, heads merged on the way out.  Replaces
 *   ScaledDotProductAttention.forward + head split / merge   reference acoustic_models/transformer.py:237-259,296-315
 * qkv [B][T][H][192] bf16 (q | k | v, 64 each); bias [B][Tp] fp32 additive key bias (0 = attend, -inf = padding), Tp = T
 * rounded up to a multiple of 32 with a -inf tail; out [B][T][H*64] bf16; lse [B*H][T] fp32 (log-sum-exp of the scaled,
 * biased scores: the backward pass recomputes the probabilities from it).  Dropout (p_drop) acts on the probabilities
 * after the softmax; masks are a counter hash of (seed word on the device, salt, (b, h, query, key)).
 * ------------------------------------------------------------------------------------------- */
int msmc_attn_fwd(const void* qkv, const float* bias, void* out, float* lse, int B, int T, int H, int Tp, float scale,
                  float p_drop, const long long* seed, long long salt, msmc_stream stream);
/* Backward: dqkv [B][T][H][192] (dq | dk | dv, every element written) from dout [B][T][H*64]; the probabilities are
 * recomputed from lse and the same dropout hash (same seed word and salt as the forward call).  dsum [B*H][T] fp32 scratch
 * (dO . O per query, written by the first of the two launches, read by the second). */
int msmc_attn_bwd(const void* qkv, const float* bias, const void* out, const float* lse, const void* dout, void* dqkv,
                  float* dsum, int B, int T, int H, int Tp, float scale, float p_drop, const long long* seed, long long salt,
                  msmc_stream stream);
/* The same two calls with fp32 storage (qkv, out, dout, dqkv fp32 in the same layouts; bias, lse, dsum as above): the
 * products run on the exact-fp32 matrix instruction and the exponentials are the accurate ones, so the fp32 parity bar
 * applies.  For the same (seed word, salt, B, T, H, p_drop) they drop exactly the entries the bf16 calls drop.  Return
 * codes as above: MSMC_E_SHAPE for Tp % 32 != 0, Tp < T or p_drop >= 1 (nothing is launched). */
int msmc_attn_fwd_f32(const float* qkv, const float* bias, float* out, float* lse, int B, int T, int H, int Tp, float scale,
                      float p_drop, const long long* seed, long long salt, msmc_stream stream);
int msmc_attn_bwd_f32(const float* qkv, const float* bias, const float* out, const float* lse, const float* dout, float* dqkv,
                      float* dsum, int B, int T, int H, int Tp, float scale, float p_drop, const long long* seed,
                      long long salt, msmc_stream stream);

/* out[q] = epilogue( sum_t sum_ci w[tap_w[t]][co][ci] * act(x[in(q, t)][ci]) + bias[co] ). */
int msmc_conv_gather(const msmc_conv_desc* desc, msmc_stream stream);
/* n (<= 16) INDEPENDENT convolutions, each with msmc_conv_gather semantics, issued in as few launches as their kernel
 * choices allow: members that resolve to the same second-generation kernel instantiation share one grid (the three
 * parallel ResBlocks of a generator stage; one layer of the five period / six resolution sub-discriminators).  Each
 * alone is a grid of tens to a few hundred workgroups; together they fill the 256 CUs. */
int msmc_conv_gather_group(const msmc_conv_desc* descs, int n, msmc_stream stream);

/* dw[tap_w[t]][co][ci] += sum_{b,q} g[b][out(q)][co] * act(x[b][in(q, t)][ci])   (fp32 atomics; caller zeroes dw).
 * Geometry fields as for the forward convolution it differentiates; desc->x = x, desc->out unused,
 * g has the forward output's shape [B][Hout][Wout][Cout] and dtype; desc->mask_slope is a leaky-ReLU
 * slope applied to g on load (1 = identity).  db (may be NULL): db[co] += sum_{b,q} g[b][out(q)][co]. */
int msmc_conv_wgrad(const msmc_conv_desc* desc, const void* g, float* dw, float* db, msmc_stream stream);
/* n (<= 16) independent weight gradients, msmc_conv_wgrad semantics each (db may be NULL, or db[i] NULL); bf16
 * second-generation members share one grid per (at most six) members. */
int msmc_conv_wgrad_group(const msmc_conv_desc* descs, const void* const* g, float* const* dw, float* const* db, int n,
                          msmc_stream stream);
/* Third generation (desc->variant == 3, bf16): NO atomics.  The pixel reduction is split only as far as it takes to fill
 * the chip; every split stores its partial dW (and db) into its own region of a caller-provided workspace with plain
 * stores, and a second launch adds the regions to dw / db in split order (bit-reproducible).  With a single split the
 * kernel accumulates straight into dw and needs no workspace.  msmc_conv_wgrad_workspace: bytes this descriptor needs
 * (0 for other variants / dtypes); a group needs the sum over its members.  MSMC_E_WORKSPACE when it is too small.
 * Fourth generation (desc->variant 4 / 5 / 6, msmc-tts_amd/csrc/wgrad4.inc): same contract and second stage; the
 * workgroup's pixel tiles (output gradient rows + the x rows all its taps touch) stream global -> LDS through a ring
 * filled by global_load_lds_dwordx4 while the matrix cores work on the previous tile.  Inside msmc_conv_wgrad_group_ws
 * such members join the shared grid as third-generation members.  Channel counts: multiples of 8 (tiles of 64 that end past the
 * channels read zeros).  desc->variant 9 (msmc-tts_amd/csrc/wgrad7.inc): the same scope and contract on 128 x 128 channel tiles,
 * eight waves per workgroup, for layers with >= 128 channels on both sides and enough pixels to fill the chip at that size (the
 * 600 <-> 1536 feed-forward layers of the predictor at B = 64); always a launch of its own inside a group call. */
size_t msmc_conv_wgrad_workspace(const msmc_conv_desc* desc, const void* g);
int msmc_conv_wgrad_ws(const msmc_conv_desc* desc, const void* g, float* dw, float* db, void* workspace,
                       size_t workspace_bytes, msmc_stream stream);
int msmc_conv_wgrad_group_ws(const msmc_conv_desc* descs, const void* const* g, float* const* dw, float* const* db, int n,
                             void* workspace, size_t workspace_bytes, msmc_stream stream);
/* As msmc_conv_wgrad_group_ws; group4 != 0: the fourth-generation members of the call share grids of their own kernel
 * (every member planned for its share of the chip, one second-stage launch for all of them) and the rest is issued as
 * msmc_conv_wgrad_group_ws would; 0 = msmc_conv_wgrad_group_ws. */
int msmc_conv_wgrad_group_ws4(const msmc_conv_desc* descs, const void* const* g, float* const* dw, float* const* db, int n,
                              void* workspace, size_t workspace_bytes, msmc_stream stream, int group4);

/* Deferred second stage.  Between msmc_conv_wgrad_defer_begin(sink, capacity) and msmc_conv_wgrad_defer_end() the
 * msmc_conv_wgrad_ws / _group_ws / _group_ws4 calls OF THE CALLING THREAD run their first stage only and append one record
 * per partial-result set to `sink` (up to `capacity`; sets that do not fit are reduced at once, as without a sink);
 * _defer_end returns the number recorded.  The workspace regions the records point into must stay untouched until
 * msmc_conv_wgrad_reduce_pending has added them up: n records in ceil(n / 16) (+ the two-level members' first level)
 * launches instead of one or two per weight gradient -- the host issues it once per backward pass of a network.  The
 * sums and their order are those of the immediate second stage (bit-identical results). */
typedef struct msmc_wg_pending {
    const float* ws;        /* nsplit partial regions of `stride` floats: dW (n_dw) then db (n_db) */
    float* mid;             /* intermediate regions of a two-level reduction (behind the partials) */
    float* dw;              /* accumulated into */
    float* db;              /* may be NULL */
    long stride, n_dw;
    int n_db, nsplit;
} msmc_wg_pending;
void msmc_conv_wgrad_defer_begin(msmc_wg_pending* sink, int capacity);
int msmc_conv_wgrad_defer_end(void);
int msmc_conv_wgrad_reduce_pending(const msmc_wg_pending* items, int n, msmc_stream stream);

/* Weight-norm (torch weight_norm, dim=0) for MANY convolutions in one launch.
 * Item i: v [A][Bc][T] fp32 contiguous (A = dim 0, the normalised axis; T = taps), g [A] fp32.
 *   prepare : w = v * (g / ||v||) written to up to two kernel layouts
 *             dst_k[tap*s_k[0] + a*s_k[1] + b*s_k[2]]  (dtype: 0 fp32, 1 bf16), inv_norm[a] = 1/||v||
 *   backward: from dw (fp32, layout s_1):  gg[a] = sum(dw*v)*inv_norm,
 *             gv = (g*inv_norm) * (dw - v * sum(dw*v) * inv_norm^2);  gb = db;
 *             dw and db are ZEROED as they are consumed (ready for the next accumulation)
 * ``items`` is a DEVICE array; item i owns blocks [block0, block0 + A) of the grid of total_blocks. */
typedef struct msmc_wn_item {
    const float* v;
    const float* g;         /* NULL: plain (not weight-normalised) layer -- w = v, gv = dW, gg / inv_norm unused */
    void* dst1;
    void* dst2;             /* may be NULL */
    float* inv_norm;        /* [A] */
    const float* dw;        /* backward: gradient wrt w in layout 1 (fp32) */
    float* gv;              /* backward: [A][Bc][T] */
    float* gg;              /* backward: [A] */
    long s1[3];
    long s2[3];
    int A, Bc, T, dtype, block0, nbias;
    float* db;              /* backward: [nbias] bias-gradient accumulator (consumed and zeroed), may be NULL */
    float* gb;              /* backward: [nbias] bias gradient out */
    int copies;             /* backward: dw / db hold this many privatised copies (0 or 1 = one), summed here */
    int tblock0;            /* msmc_wn_prepare_multi_tiled: first tile-block of this item (see there) */
    long dw_copy_stride;    /* elements between copies of dw */
    long db_copy_stride;    /* elements between copies of db */
} msmc_wn_item;

int msmc_wn_prepare_multi(const msmc_wn_item* items, int nitems, int total_blocks, msmc_stream stream);
/* Same result in two launches: the row pass writes layout 1 and inv_norm, then a tiled pass writes layout 2 -- the
 * transpose of the parameter's own order -- through LDS with 64 consecutive elements per store instead of one 2-byte store
 * per cache line.  Item i owns tile-blocks [tblock0, tblock0 + ceil(A/64) * ceil(Bc/16)) of total_tile_blocks (items
 * without dst2 own none); T <= MSMC_CONV_MAX_TAPS. */
int msmc_wn_prepare_multi_tiled(const msmc_wn_item* items, int nitems, int total_blocks, int total_tile_blocks,
                                msmc_stream stream);
/* Round 6: both layouts from ONE read of the parameters.  A norms-only row pass over the weight-normalised rows and a tiled
 * pass in which a workgroup reads a tile of rows x columns x all taps in the parameter's own order and writes it out twice --
 * layout 1 with b fastest, layout 2 with a fastest: both must have unit stride there (s1[2] == 1, s2[1] == 1), dst2 may be NULL.
 * Item i owns tile-blocks [tblock0, tblock0 + msmc_wn_tile_blocks(A, Bc, T)) of total_tile_blocks; ``max_taps`` = the largest T
 * among the items (sizes the tile buffer), <= MSMC_CONV_MAX_TAPS.  Device index maps replace the per-workgroup search of the
 * item table: row_item[r] = item of row r (r as block0 counts rows, total_blocks entries), norm_rows[k] = the k-th row of a
 * weight-normalised item (n_norm_rows entries, 0: no such item -- no row pass), tile_item[t] = item of tile-block t (may be NULL:
 * searched).  Replaces msmc_wn_prepare_multi_tiled's row pass (strided re-read of v, a workgroup per row) and its 64 x 16
 * transposing pass: the autoencoder's 36.7 M weights 91 + 138 us -> profiles/README.md. */
int msmc_wn_tile_blocks(int A, int Bc, int T);
int msmc_wn_prepare_multi_tiles(const msmc_wn_item* items, int nitems, int total_blocks, int total_tile_blocks, int max_taps,
                                const int* row_item, const int* norm_rows, int n_norm_rows, const int* tile_item,
                                msmc_stream stream);
int msmc_wn_backward_multi(const msmc_wn_item* items, int nitems, int total_blocks, msmc_stream stream);
/* accumulate != 0: gv / gg / gb += instead of = (a second backward before the gradients were reset: torch .grad semantics) */
int msmc_wn_backward_multi_acc(const msmc_wn_item* items, int nitems, int total_blocks, int accumulate, msmc_stream stream);
/* the same with the longest normalised row (Bc * T parameters) of the items given: rows of up to 4096 parameters run with 128
 * work-items per row and a row buffer sized to max_row -- up to 16 instead of 6 rows in flight per CU (the pass is a chain of
 * memory round trips per row) */
int msmc_wn_backward_multi_rows(const msmc_wn_item* items, int nitems, int total_blocks, int accumulate, int max_row,
                                msmc_stream stream);

/* Backward of ReflectionPad2d(p) fused with the leaky-ReLU' mask, channels-last:
 *   gx[b][y][x][c] = (sum of gp over the padded positions that reflect onto (y, x)) * (mask_src > 0 ? 1 : slope)
 * gp [B][H+2p][W+2p][C], gx and mask_src [B][H][W][C] (mask_src may be NULL). */
int msmc_reflect_fold(const void* gp, const void* mask_src, void* gx, int B, int H, int W, int C, int p, float slope,
                      int dtype, msmc_stream stream);

/* gx = g * (y > 0 ? 1 : slope): backward of a leaky ReLU from its OUTPUT y (sign-preserving), n elements. */
int msmc_lrelu_bwd(const void* g, const void* y, void* gx, long n, float slope, int dtype, msmc_stream stream);

/* Multi-tensor forms of the two helpers above: n (<= 6) tensors per launch (the same layer of all resolution
 * sub-discriminators), 16-byte channel vectors where every member allows. */
int msmc_reflect_fold_multi(const void* const* gp, const void* const* mask_src, void* const* gx, const int* B, const int* H,
                            const int* W, const int* C, int n, int p, float slope, int dtype, msmc_stream stream);
/* as msmc_reflect_fold_multi with a third input per tensor: gx = fold(gp) * lrelu'(mask_src) + res  (res[k] may be NULL):
 * the gradient of a second consumer of the padded layer's input (a feature-matching tap) without a separate add. */
int msmc_reflect_fold_multi_res(const void* const* gp, const void* const* mask_src, const void* const* res, void* const* gx,
                                const int* B, const int* H, const int* W, const int* C, int n, int p, float slope, int dtype,
                                msmc_stream stream);
/* as msmc_reflect_fold_multi_res with the third input added BEFORE the mask: gx = (fold(gp) + tap) * lrelu'(mask_src).
 * For a padded layer whose input is an ACTIVATED map with a second reader (the resolution discriminators' feature
 * maps, reference msmctts/networks/hifigan/discriminator.py DiscriminatorR.forward: the in-place leaky ReLU makes the
 * stored map the activated one): the producer's leaky-ReLU backward happens here instead of in a launch of its own. */
int msmc_reflect_fold_multi_tap(const void* const* gp, const void* const* mask_src, const void* const* tap, void* const* gx,
                                const int* B, const int* H, const int* W, const int* C, int n, int p, float slope, int dtype,
                                msmc_stream stream);
int msmc_lrelu_bwd_multi(const void* const* g, const void* const* y, void* const* gx, const long* nelem, int n, float slope,
                         int dtype, msmc_stream stream);


/* Column sums: out[c] = sum_rows g[row][c] (bias gradients); g dtype as above, out fp32 (overwritten). */
int msmc_colsum(const void* g, float* out, long rows, int C, int dtype, msmc_stream stream);
/* The same without atomics (bit-reproducible): per-block partial sums into ``workspace`` (msmc_colsum_workspace bytes), then a
 * fixed-order sum; accumulate != 0: out += (the bias-gradient accumulators of a bank).  Two launches. */
size_t msmc_colsum_workspace(long rows, int C);
int msmc_colsum_ws(const void* g, float* out, long rows, int C, int dtype, int accumulate, void* workspace,
                   size_t workspace_bytes, msmc_stream stream);

/* ---------------------------------------------------------------------------------------------
 * D3/L1  spectral front-ends as framed-DFT GEMMs on the matrix cores (exact-fp32 MFMA through
 * msmc_conv_gather with one tap) plus three fused element-wise kernels.  Replaces torch.stft (cuFFT/hipFFT)
 * and the surrounding glue of
 *   TorchSTFT.transform / MelScale.forward   reference msmctts/utils/audio.py:398-419, 348-376
 *   MelLoss.mel_spectrogram                  reference msmctts/trainers/criterions/stft_loss.py:76-108
 * All fp32.
 * ------------------------------------------------------------------------------------------- */

/* frames[b][t][j] = x[b][reflect(t*hop + j - pad)] for j < n_fft, 0 for n_fft <= j < NP (row pitch NP).
 * pad = n_fft/2 (centred STFT) or (n_fft-hop)/2 (MelLoss); x [B][L], frames [B][T][NP].  The reflection folds once on each
 * side: both entries (and kinds 0 / 1 of msmc_spectral_multi) return MSMC_E_SHAPE unless L > pad and the last position read,
 * (T-1)*hop + n_fft - 1 - pad, is at most 2L - 2. */
int msmc_stft_frames_fwd(const float* x, float* frames, int B, int L, int T, int n_fft, int NP, int hop, int pad,
                         msmc_stream stream);
/* overlap-add adjoint: gx[b][l] = sum of gframes over every (t, j) that read sample l (reflections included). */
int msmc_stft_frames_bwd(const float* gframes, float* gx, int B, int L, int T, int n_fft, int NP, int hop, int pad,
                         msmc_stream stream);

/* spec [R][CP] holds re in columns [0,F) and im in [F,2F) -> mag[r][f] = sqrt(clamp(re^2+im^2, lo)) when
 * clamp_mode = 1 (audio.py:403-404) or sqrt(re^2+im^2+lo) when clamp_mode = 0 (stft_loss.py:104);
 * mag [R][FP], columns F..FP zeroed. */
int msmc_spec_mag_fwd(const float* spec, float* mag, long R, int F, int CP, int FP, float lo, int clamp_mode,
                      msmc_stream stream);
int msmc_spec_mag_bwd(const float* spec, const float* mag, const float* gmag, float* gspec, long R, int F, int CP,
                      int FP, float lo, int clamp_mode, msmc_stream stream);

/* MRD image, channels-last [B][F][T][2] from mel [B*T][FP]: ch0 = mel, ch1 = clamp((20 log10(mel) - ref + 100)/100, 0, 1)
 * (audio.py:411-419 'double' domain, ref_level_db = 20, min_level_db = -100). */
int msmc_mrd_image_fwd(const float* mel, float* img, int B, int T, int F, int FP, msmc_stream stream);
/* the same with the image (and its gradient) in the discriminator stack's compute dtype: 0 fp32, 1 bf16 */
int msmc_mrd_image_fwd_dt(const float* mel, void* img, int B, int T, int F, int FP, int dtype, msmc_stream stream);
int msmc_mrd_image_bwd_dt(const float* mel, const void* gimg, float* gmel, int B, int T, int F, int FP, int dtype,
                          msmc_stream stream);
int msmc_mrd_image_bwd(const float* mel, const float* gimg, float* gmel, int B, int T, int F, int FP,
                       msmc_stream stream);
/* One channel of that image alone, channels-last [B][F][T][1] ('linear' domain: channel = 0, the magnitude; 'log' domain:
 * channel = 1, the normalised log-magnitude): the forward value is that channel of msmc_mrd_image_fwd_dt bit for bit, the other
 * channel is neither computed nor stored; the gradient of channel 1 is zero where the clamp is active. */
int msmc_mrd_image1_fwd_dt(const float* mel, void* img, int B, int T, int F, int FP, int channel, int dtype, msmc_stream stream);
int msmc_mrd_image1_bwd_dt(const float* mel, const void* gimg, float* gmel, int B, int T, int F, int FP, int channel, int dtype,
                           msmc_stream stream);

/* Waveform fan-out of the discriminator (reference msmctts/networks/hifigan/discriminator.py:102-116,135-145,180-190): the period
 * sub-discriminators read the waveform cast to the stack's dtype and reflection-padded on the right to a multiple of their
 * period; the resolution sub-discriminators read it in fp32.  Forward: copies[k] [B][padded_len[k]] (dtype 0 fp32 / 1 bf16),
 * L <= padded_len[k] <= 2L - 1, all n (<= 8) copies in one launch.  Backward: gy [B][L] fp32 = sum of the n32 (<= 8) fp32
 * gradients g32[j] [B][L] and of the copies' gradients folded at the reflected tail (entries may be NULL: no gradient) -- one
 * launch instead of two pad gradients, a cast gradient and ~20 accumulations by the autograd engine. */
int msmc_wave_fan_fwd(const float* y, void* const* copies, const int* padded_len, int n, int B, int L, int dtype,
                      msmc_stream stream);
int msmc_wave_fan_bwd(const float* const* g32, int n32, const void* const* gcopies, const int* padded_len, int n, float* gy,
                      int B, int L, int dtype, msmc_stream stream);
/* Several element-wise stages of the spectral front-ends in ONE launch (the resolution discriminators' five chains advance in lock
 * step: five framings, five magnitudes, five images -- forward and backward).  kind: 0 msmc_stft_frames_fwd (a = x, out = frames),
 * 1 _bwd (a = gframes, out = gx), 2 msmc_spec_mag_fwd (a = spec, out = mag), 3 _bwd (a = spec, b = mag, c = gmag, out = gspec),
 * 4 msmc_mrd_image_fwd_dt (a = mel, out = img), 5 _bwd_dt (a = mel, b = gimg, out = gmel), 6 msmc_log_clamp_fwd (a = x, out = y, R = n),
 * 7 _bwd (a = x, b = g, out = gx, R = n), 8 msmc_mrd_image1_fwd_dt (a = mel, out = img, channel), 9 _bwd_dt (a = mel, b = gimg,
 * out = gmel, channel); the remaining fields are the arguments of those entry points. */
#define MSMC_SPECTRAL_MULTI_MAX 8
typedef struct msmc_spectral_op {
    int kind, dtype;
    const void* a;
    const void* b;
    const void* c;
    void* out;
    int B, L, T, n_fft, NP, hop, pad;
    int F, CP, FP, clamp_mode;
    float lo;
    long R;
    int channel;
} msmc_spectral_op;
int msmc_spectral_multi(const msmc_spectral_op* ops, int n, msmc_stream stream);
/* Vocoder windows of a captured step (reference msmctts_trainer.py:211-219, window starts on the device): frames[b][i] = starts[b] + i
 * (int64, i < nframes) and target[b][j] = wav[b][starts[b] * hop + j] (j < nframes * hop; wav [B][L] fp32).  The caller guarantees
 * starts[b] * hop + nframes * hop <= L (VQGANTrainer checks the batch on the host). */
int msmc_window_gather(const long* starts, const float* wav, long* frames, float* target, int B, int nframes, int hop, long L,
                       msmc_stream stream);
/* Windows of a SUBSET of utterances (reference emb_vqgan_trainer.py:41-56: n <= B sampled utterances, one window each), csrc/window.hip.
 * x [B][T][C], win [n][2] int32 on the device = (utterance u_j, first row s_j), out [n][W][C] -- the channels-last [n, 1, W, C]
 * image a convolution stack reads; *_bf16: 0 = fp32, 1 = bf16 for that tensor.  out[j][t][c] = x[u_j][s_j + t][c], converted
 * with round-to-nearest-even (the bits of torch.Tensor.to); a row s_j + t outside [0, T) or an utterance outside [0, B) is never
 * read and gives zeros, so any table contents are safe.
 * Backward: EVERY element of gx [B][T][C] is written exactly once with plain stores -- gout of the window row that covers it,
 * zero otherwise (no atomics, no zero-fill launch before it).  Caller's contract: the u_j are strictly increasing; when broken,
 * which window wins is unspecified but no access leaves the buffers.
 * C % 8 == 0 (and 16-byte aligned pointers): 16-byte accesses; any other C >= 1: one element per access.
 * MSMC_E_SHAPE (nothing is launched) for W < 1, n < 1, n > B, C < 1, T < 1. */
int msmc_window_gather_fwd(const void* x, int x_bf16, const int* win, void* out, int out_bf16, int B, int T, int C, int n, int W,
                           msmc_stream stream);
int msmc_window_gather_bwd(const void* gout, int gout_bf16, const int* win, void* gx, int gx_bf16, int B, int T, int C, int n, int W,
                           msmc_stream stream);

/* y = log(max(x, lo)) and its backward gx = g * (x > lo ? 1/x : 0) over n elements (stft_loss.py:110-114). */
int msmc_log_clamp_fwd(const float* x, float* y, long n, float lo, msmc_stream stream);
int msmc_log_clamp_bwd(const float* x, const float* g, float* gx, long n, float lo, msmc_stream stream);

/* ---------------------------------------------------------------------------------------------
 * T2  GAN loss terms over MANY tensors in one launch (feature matching has 55 map pairs, the LSGAN terms
 * 10 score tensors): replaces the per-tensor l1_loss / MSELoss loops of
 *   VQGANTrainer.train_step, reference msmctts/trainers/msmctts_trainer.py:165-171,187-193.
 * Tensors are dense (any permutation of a contiguous layout; a and b share it); dtype 0 fp32 / 1 bf16.
 * ------------------------------------------------------------------------------------------- */
#define MSMC_MAX_TENSORS 64
typedef struct msmc_tensor_table {
    const void* a[MSMC_MAX_TENSORS];
    const void* b[MSMC_MAX_TENSORS];      /* second operand (L1) or unused */
    void* ga[MSMC_MAX_TENSORS];           /* backward: gradient wrt a */
    long n[MSMC_MAX_TENSORS];
    int count, dtype;
} msmc_tensor_table;

/* out[0] = sum_i mean_e |a_i[e] - b_i[e]| */
int msmc_l1_multi_fwd(const msmc_tensor_table* t, float* out, msmc_stream stream);
/* ga_i[e] = gout[0] * sign(a_i[e] - b_i[e]) / n_i */
/* the same forward sums without atomics: per-block partial sums into ``partial`` (msmc_loss_multi_parts() floats), added by one
 * workgroup in a fixed order (tensor by tensor, block by block): bit-reproducible, and no thousands of same-address atomics */
int msmc_loss_multi_parts(void);
int msmc_l1_multi_fwd_ws(const msmc_tensor_table* t, float* partial, float* out, msmc_stream stream);
int msmc_mse_const_multi_fwd_ws(const msmc_tensor_table* t, float target, float* partial, float* out, msmc_stream stream);
int msmc_l1_multi_bwd(const msmc_tensor_table* t, const float* gout, msmc_stream stream);
/* out[0] = sum_i mean_e (a_i[e] - target)^2 ;  ga_i[e] = gout[0] * 2 (a_i[e] - target) / n_i */
int msmc_mse_const_multi_fwd(const msmc_tensor_table* t, float target, float* out, msmc_stream stream);
int msmc_mse_const_multi_bwd(const msmc_tensor_table* t, float target, const float* gout, msmc_stream stream);

/* Weighted sums of loss scalars: out[0] = sum_i weights[i] * terms[i][0] (terms: n <= 64 device pointers to fp32 scalars; weights:
 * n HOST floats, copied into the launch), in term order; backward gvec[i] = gout[0] * weights[i].  Replaces the multiply-and-add
 * chains of 0-dim tensors of reference msmctts_trainer.py:52-62,129-133,160-195 (one launch per sum instead of two per term). */
int msmc_scalar_wsum_fwd(const float* const* terms, const float* weights, int n, float* out, msmc_stream stream);
int msmc_scalar_wsum_bwd(const float* gout, const float* weights, int n, float* gvec, msmc_stream stream);

/* Length-masked means over [B][T][C] tensors (rows t >= lengths[b] are padding): the scalar terms
 *   QuantizerLoss                      reference msmctts/trainers/msmctts_trainer.py:52-62
 *   frame loss                         reference msmctts/trainers/msmctts_trainer.py:129-133
 *   'mse' embedding loss               reference msmctts/networks/vqgantts/msmc_vqgan.py:228-247
 * as two launches forward (partial sums over the valid rows, then a fixed-order sum: bit-reproducible) and one backward,
 * instead of ~10 stock kernels per term.  mode 0: out[0] = sum_valid a / sum_b lengths[b] / C; mode 1: the same over
 * (a - b)^2.  a / b dtype codes 0 fp32, 1 bf16 (mode 0 ignores b); lengths int64 (len_is_64) or int32.  partial: fp32
 * scratch of msmc_masked_mean_parts(B) floats; out: fp32[2] ([1] = 1 / (sum lengths * C), read by the backward pass).
 * Backward: ga = gout[0] * d out[0] / d a (zeros on padding rows), gb = -ga; either may be NULL. */
int msmc_masked_mean_parts(int B);
int msmc_masked_mean_fwd(const void* a, const void* b, const void* lengths, int len_is_64, int B, int T, int C, int a_dtype,
                         int b_dtype, int mode, float* partial, float* out, msmc_stream stream);
int msmc_masked_mean_bwd(const void* a, const void* b, const void* lengths, int len_is_64, int B, int T, int C, int a_dtype,
                         int b_dtype, int mode, const float* out, const float* gout, void* ga, void* gb, msmc_stream stream);

/* Triple (hinge) loss of predictor training against a frozen codebook (BASELINE configuration #4): Quantize.compute_triple_loss,
 * reference msmctts/networks/vqgantts/modules.py:86-116, for all heads of a MultiHeadQuantize (:152-168) in one launch.
 *   p [N][D] fp32 predictions, trg [N][H] int64 target indices, embed_t [H][K][D/H] / enorm [H][K] from msmc_vq_prepare;
 *   lossh [N][H] = reduce_k [t_k != 0] max(t_k + margin, 0) / d,  t_k = sum_c (p_c - e_trg,c)^2 - ((|p|^2 - 2 p.e_k) + |e_k|^2),
 *   reduce = sum (mean == 0) or mean over the K codewords;  gp [N][D] = d lossh[n][h] / d p (the caller scales it by the
 *   incoming gradient and takes the mean over heads).  d = D/H in {16, 32, 64, 128}; (K d + K) floats of LDS. */
int msmc_triple_loss(const float* p, const int64_t* trg, const float* embed_t, const float* enorm, float* lossh, float* gp, int N,
                     int D, int H, int K, float margin, int mean, msmc_stream stream);

/* The same loss with no resident codebook (msmc-tts_amd/csrc/triple_stream.inc): every head's rows and norms pass through LDS
 * in double-buffered chunks of `chunk` codewords while a workgroup keeps its frames.  Same expressions and outputs; the order
 * of every fp32 sum depends on (d, K) alone -- not on the chunk or the grid.  On every head shape msmc_triple_loss takes it is
 * that kernel's (one lane per frame): lossh and gp are bit-identical to it.  Beyond those shapes a frame's channels are split
 * over L lanes (4 for d = 128, 8 for d = 256 / 512) and the active rows are added in blocks of 8 codewords with compensated block sums.  d = D/H in {16, 32, 64, 128, 256, 512}, any K >= 1.  chunk = 0: the launcher's choice (the largest
 * multiple of 8 that keeps the two buffers under 80 KiB, at most 64); chunk > 0: forced (larger than K means K).  Returns
 * MSMC_E_SHAPE for another d, p / embed_t / gp not 16-byte aligned, chunk < 0 or two buffers of 2 chunk (d + 1) floats beyond
 * 160 KiB; 0 at once, with no launch, for N == 0. */
int msmc_triple_loss_stream(const float* p, const int64_t* trg, const float* embed_t, const float* enorm, float* lossh, float* gp,
                            int N, int D, int H, int K, float margin, int mean, int chunk, msmc_stream stream);

/* The same loss for ONE wide head, GEMM-shaped (msmc-tts_amd/csrc/triple_wide.inc): the k-means unit codebooks (d = 768 / 1024,
 * K = 100 .. 2000) neither kernel above takes.  Operands and outputs as msmc_triple_loss with H = 1 (embed_t [K][d] / enorm [K]
 * from msmc_vq_prepare, lossh [N], gp [N][d]).  Two launches on fp32 MFMA: the K products p.e_k of a frame tile, the hinge
 * decisions, lossh and a bit mask of the active codewords (the workspace: 8 bytes per frame and 64 codewords,
 * msmc_triple_loss_wide_workspace, 0 for N <= 0 or a shape the kernel refuses); then mask x embed_t per (frame tile, 128
 * channels).  The target's own row never enters the gradient.  The active t_k + margin are added before the one
 * multiplication by 1 / d (1 / (d K) for the mean); the gradient rows add up per 64 codewords, those sums in a compensated
 * sum.  The order of every fp32 sum depends on (d, K) alone -- not on N or the grid; no atomics.  Takes d % 16 == 0,
 * 16 <= d <= 2048, K >= 1; MSMC_E_SHAPE otherwise or for p / embed_t / gp not 16-byte aligned, nothing launched; 0 at once,
 * with no launch, for N == 0; MSMC_E_WORKSPACE for a workspace below msmc_triple_loss_wide_workspace. */
size_t msmc_triple_loss_wide_workspace(int N, int d, int K);
int msmc_triple_loss_wide(const float* p, const int64_t* trg, const float* embed_t, const float* enorm, float* lossh, float* gp,
                          int N, int d, int K, float margin, int mean, void* workspace, size_t workspace_bytes,
                          msmc_stream stream);

/* ---------------------------------------------------------------------------------------------
 * E1/V3  fused element-wise / row-normalisation kernels of the FFT blocks and the quantiser glue (csrc/norm.hip).
 * Replace the stock-kernel chains behind
 *   layer_norm(dropout(h) + residual) [* non_pad_mask]   reference acoustic_models/transformer.py:262-266, 318-323, 352-356
 *   tanh(a) * sigmoid(b) (+ dropout)                     reference vqgantts/modules.py:172-179, 241
 *   Tanh of the 1x1 stacks                               reference vqgantts/msmc_vqgan.py:115-136
 * Rows [N][C] fp32 (dtype 0) / bf16 (dtype 1); statistics and parameter gradients fp32.  Dropout masks are functions of
 * (seed[0] on the device, salt, element index): nothing is stored, both passes regenerate them; seed may be NULL when
 * p_drop == 0.  C <= 1024.
 * ------------------------------------------------------------------------------------------- */
/* v = drop(x) + res (res may be NULL); y = LayerNorm(v) * gamma + beta, rows with keep_row[n] == 0 zeroed (keep_row may be
 * NULL); v, mean [N], rstd [N] are kept for the backward pass.  Any contiguous rows are taken: four-element vector accesses
 * where C % 4 == 0 and x / res / y / v are 16-byte (fp32) / 8-byte (bf16) and gamma / beta 16-byte aligned, element accesses
 * otherwise.  MSMC_E_SHAPE for C > 1024 or p_drop outside [0, 1). */
int msmc_add_ln_fwd(const void* x, const void* res, const float* gamma, const float* beta, const unsigned char* keep_row,
                    void* y, void* v, float* mean, float* rstd, long N, int C, float eps, float p_drop,
                    const long long* seed, long long salt, int dtype, msmc_stream stream);
/* The attention sub-layer's tail in one launch (bf16): y = layer_norm(dropout(a W^T + bias) + res) * keep_row with the same mask
 * hash, saved tensors (v, mean, rstd) and rounding points as msmc_conv_gather (1 tap) followed by msmc_add_ln_fwd -- reference
 * acoustic_models/transformer.py:259-266.  a [N][K], W [C][K] bf16 (the projection's forward slice), bias fp32 [C] (required),
 * res / y / v [N][C] bf16; K % 32 == 0, C % 4 == 0, C <= 640.  The backward pass is the two-launch chain's (msmc_add_ln_bwd, then the
 * projection's data / weight gradient). */
int msmc_fc_add_ln_fwd(const void* a, const void* W, const float* bias, const void* res, const float* gamma, const float* beta,
                       const unsigned char* keep_row, void* y, void* v, float* mean, float* rstd, long N, int C, int K, float eps,
                       float p_drop, const long long* seed, long long salt, msmc_stream stream);
size_t msmc_add_ln_bwd_workspace(long N, int C);
/* gx = d/dx, gres = d/dres (may be NULL), dgamma / dbeta fp32 [C] (accumulate != 0: +=), fixed reduction order.
 * dgamma == dbeta == NULL: only the per-workgroup partials are produced -- they stay in `workspace`
 * ([ceil(N / 16)][2][C] fp32, which the caller then keeps) for msmc_add_ln_param_multi.  Alignment as msmc_add_ln_fwd (g / v / gx /
 * gres and gamma: the element path where one of them does not start on a four-element boundary).  MSMC_E_SHAPE for C > 1024 or
 * p_drop outside [0, 1), as the forward entry; MSMC_E_WORKSPACE below msmc_add_ln_bwd_workspace. */
int msmc_add_ln_bwd(const void* g, const void* v, const float* mean, const float* rstd, const float* gamma,
                    const unsigned char* keep_row, void* gx, void* gres, float* dgamma, float* dbeta, void* workspace,
                    size_t workspace_bytes, long N, int C, float p_drop, const long long* seed, long long salt, int accumulate,
                    int dtype, msmc_stream stream);
/* The parameter gradients of several LayerNorms from the partials their msmc_add_ln_bwd calls left behind, in launches of up
 * to MSMC_LN_PARAM_MAX items (the 24 LayerNorms of the FFT stacks: one launch at the end of the backward pass instead of one
 * 10 us launch behind every LayerNorm backward, on the critical path of the block chain).  `items` is a HOST array (passed to
 * the kernel by value); same fixed reduction order as msmc_add_ln_bwd's own second stage; two items must not name the same
 * dgamma / dbeta.  Reference: the weight / bias gradients autograd derives for nn.LayerNorm in
 * acoustic_models/transformer.py:270-288,330-352. */
#define MSMC_LN_PARAM_MAX 32
typedef struct {
    const float* part;      /* the workspace of the msmc_add_ln_bwd call: [nblocks][2][C] */
    float* dgamma;
    float* dbeta;
    int nblocks;            /* ceil(N / 16) of that call */
    int C;
    int accumulate;         /* != 0: += */
    int reserved;
} msmc_ln_param_item;
int msmc_add_ln_param_multi(const msmc_ln_param_item* items, int nitems, msmc_stream stream);
/* Head of FFTBlocks.forward (reference msmctts/networks/acoustic_models/transformer.py:375-395) with the positions of
 * vqgantts/msmc_vqgan.py:56-58 folded in: out[b][t][:] = seq[b][t][:] + table[t < len[b] ? t + 1 : 0][:] (seq / out
 * [B][T][C] in in_dtype / out_dtype, table fp32 [table_rows][C], T + 1 <= table_rows), keep_row[b T + t] = t < len[b],
 * key_bias (may be NULL) [B][Tp] = 0 on real frames, -inf on padding and on the tail T .. Tp - 1 (T <= Tp < T + 64: MSMC_E_SHAPE
 * otherwise).  lengths: int32 or int64.  Vector accesses where C % 4 == 0 and seq / out / table start on a four-element boundary
 * of their dtype (table: 16 bytes), element accesses otherwise. */
int msmc_fft_prologue(const void* seq, const void* lengths, int len_is_64, const float* table, int table_rows, void* out,
                      unsigned char* keep_row, float* key_bias, int B, int T, int C, int Tp, int in_dtype, int out_dtype,
                      msmc_stream stream);
/* x [N][2C] -> y [N][C] = drop(tanh(x[:, :C]) * sigmoid(x[:, C:])); backward recomputes from x.  Both entries: MSMC_E_SHAPE for
 * p_drop outside [0, 1). */
int msmc_gate_fwd(const void* x, void* y, long N, int C, float p_drop, const long long* seed, long long salt, int dtype,
                  msmc_stream stream);
int msmc_gate_bwd(const void* x, const void* g, void* gx, long N, int C, float p_drop, const long long* seed, long long salt,
                  int dtype, msmc_stream stream);
/* Element-wise glue of the quantiser and of the generator's backward pass (round 6; dtype 0 fp32 / 1 bf16, n % 4 == 0, operands
 * 16-byte (fp32) / 8-byte (bf16) aligned).
 *   msmc_sum_n: out = ((a + b) + c) + d, c and d optional -- the input gradients of the parallel ResBlocks (hifigan/generator.py:47-52);
 *   msmc_dropout_add_fwd: y = dropout(x) + res (res optional) with the counter-hash masks of msmc_add_ln_fwd (element index = position),
 *   msmc_dropout_bwd: gx = g * mask * scale -- F.dropout + the residual adds of vqgantts/msmc_vqgan.py:141-176;
 *   msmc_row_mask: keep[b][t] = (t < lengths[b]) as 1 / 0 in ``dtype`` -- ~get_mask_from_lengths (utils/utils.py:9-16) cast to the compute dtype. */
int msmc_sum_n(const void* a, const void* b, const void* c, const void* d, void* out, long n, int dtype, msmc_stream stream);
int msmc_dropout_add_fwd(const void* x, const void* res, void* y, long n, float p_drop, const long long* seed, long long salt, int dtype,
                         msmc_stream stream);
int msmc_dropout_bwd(const void* g, void* gx, long n, float p_drop, const long long* seed, long long salt, int dtype, msmc_stream stream);
int msmc_row_mask(const void* lengths, int lengths_are_int64, void* keep, int B, int T, int dtype, msmc_stream stream);
/* y = tanh(x); gx = g * (1 - y*y) over n elements. */
int msmc_tanh_fwd(const void* x, void* y, long n, int dtype, msmc_stream stream);
int msmc_tanh_bwd(const void* y, const void* g, void* gx, long n, int dtype, msmc_stream stream);
/* y (fp32) = tanh(x) for x in the compute dtype (``dtype``: 0 fp32, 1 bf16) -- the vocoder's output activation, reference
 * hifigan/generator.py:52-54 -- and its backward gx (compute dtype) = g (fp32) * (1 - y^2) */
int msmc_tanh_f32_fwd(const void* x, float* y, long n, int dtype, msmc_stream stream);
int msmc_tanh_f32_bwd(const float* y, const float* g, void* gx, long n, int dtype, msmc_stream stream);
/* BatchNorm over frames: nn.BatchNorm1d(C, eps, momentum, affine=False) of the normalised quantiser (``norm: True``, reference
 * vqgantts/msmc_vqgan.py:115-123, 177-178) on channels-last rows x [N][C] (``dtype``: 0 fp32, 1 bf16), statistics per channel
 * over all N rows in fp32.  C % 8 == 0 and C <= 1024, x / y / g / gx / mean / rstd / workspace 16-byte aligned, N < 2^31:
 * MSMC_E_SHAPE otherwise.  Every sum runs in a fixed order (no atomics): two calls on the same input are bit-identical.
 * Bytes of scratch the two training passes need for these sizes (0 for a refused shape). */
size_t msmc_bn_workspace(long N, int C);
/* Training forward, two launches: per-slab (count, mean, M2) into the workspace (Welford; never E[x^2] - E[x]^2), then Chan's
 * merge of the slabs and y = (x - mean) * rstd with the biased variance.  y is written in ``out_dtype``: ``dtype`` or 0 (fp32 for
 * the fp32 VQ search behind it).  mean / rstd [C] fp32 are kept for the backward pass; running_mean / running_var (both or
 * neither) are blended with ``momentum`` (running_var from the unbiased variance) and num_batches_tracked (int64, may be NULL)
 * is incremented, all on the device.  N < 2: MSMC_E_SHAPE (one value per channel has no variance). */
int msmc_bn_fwd(const void* x, void* y, float* mean, float* rstd, float* running_mean, float* running_var,
                long long* num_batches_tracked, void* workspace, size_t workspace_bytes, long N, int C, float eps, float momentum,
                int dtype, int out_dtype, msmc_stream stream);
/* Evaluation forward, one launch: y = (x - running_mean) / sqrt(running_var + eps); rstd [C] (may be NULL) receives
 * 1 / sqrt(running_var + eps) for the evaluation backward. */
int msmc_bn_eval_fwd(const void* x, const float* running_mean, const float* running_var, void* y, float* rstd, long N, int C,
                     float eps, int dtype, int out_dtype, msmc_stream stream);
/* Training backward, two launches: per-slab sum(g) and sum(g * xhat) into the workspace, then
 * gx = rstd * (g - sum(g) / N - xhat * sum(g * xhat) / N) in ``dtype``; g in ``g_dtype``: ``dtype`` or 0 (fp32). */
int msmc_bn_bwd(const void* g, const void* x, const float* mean, const float* rstd, void* gx, void* workspace,
                size_t workspace_bytes, long N, int C, int g_dtype, int dtype, msmc_stream stream);
/* Evaluation backward: gx = g * rstd, with the rstd the evaluation forward wrote. */
int msmc_bn_eval_bwd(const void* g, const float* rstd, void* gx, long N, int C, int g_dtype, int dtype, msmc_stream stream);

/* ---------------------------------------------------------------------------------------------
 * The speaker reference encoder's own operators (csrc/tdnn.hip): ECAPA-TDNN, reference msmctts/networks/vqgantts/tdnn.py:67-244.
 * Channels-last activations (``dtype``: 0 fp32, 1 bf16), statistics / sums / parameters and their gradients fp32; activation
 * pointers, per-channel vectors and workspaces 16-byte aligned; every sum in a fixed order (no atomics): two calls on the same
 * input are bit-identical.  MSMC_E_SHAPE for anything outside the stated constraints.
 * ------------------------------------------------------------------------------------------- */
/* ReLU + affine BatchNorm, bn(F.relu(conv(x))) with nn.BatchNorm1d defaults (tdnn.py:96-98, 115-116):
 *   y = gamma * (relu(x) - mean) * rstd + beta  over rows x [N][C] at a row stride of ``ldx`` elements (ld >= C, ld % 8 == 0: a
 *   channel slice of a wider row, as the Res2 branches normalise), y at ``ldy``.  C % 8 == 0, C <= 1024, N < 2^31.
 * Bytes of scratch of the two-launch passes (0 for a refused shape). */
size_t msmc_relu_bn_workspace(long N, int C);
/* Training forward, two launches: per-slab Welford (count, mean, M2) of relu(x), then Chan's merge and the normalisation.  mean /
 * rstd [C] are kept for the backward pass; running_mean / running_var (both or neither; unbiased variance) and
 * num_batches_tracked (int64, may be NULL) advance on the device.  N < 2: MSMC_E_SHAPE. */
int msmc_relu_bn_fwd(const void* x, long ldx, const float* gamma, const float* beta, void* y, long ldy, float* mean, float* rstd,
                     float* running_mean, float* running_var, long long* num_batches_tracked, void* workspace,
                     size_t workspace_bytes, long N, int C, float eps, float momentum, int dtype, msmc_stream stream);
/* Evaluation forward, one launch, from the running statistics; rstd [C] (may be NULL) receives 1 / sqrt(running_var + eps). */
int msmc_relu_bn_eval_fwd(const void* x, long ldx, const float* gamma, const float* beta, const float* running_mean,
                          const float* running_var, void* y, long ldy, float* rstd, long N, int C, float eps, int dtype,
                          msmc_stream stream);
/* Training backward, two launches; the ReLU mask is recomputed from x, xhat = (relu(x) - mean) * rstd:
 *   dbeta = sum g, dgamma = sum g xhat, gx = [x > 0] gamma rstd (g - dbeta / N - xhat dgamma / N); g at ``ldg``, gx at ``ldgx``. */
int msmc_relu_bn_bwd(const void* g, long ldg, const void* x, long ldx, const float* mean, const float* rstd, const float* gamma,
                     void* gx, long ldgx, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, long N, int C,
                     int dtype, msmc_stream stream);
/* Evaluation backward: gx = [x > 0] gamma rstd g in one launch; with dgamma / dbeta (both or neither, then with the workspace)
 * the per-slab sums run first. */
int msmc_relu_bn_eval_bwd(const void* g, long ldg, const void* x, long ldx, const float* running_mean, const float* rstd,
                          const float* gamma, void* gx, long ldgx, float* dgamma, float* dbeta, void* workspace,
                          size_t workspace_bytes, long N, int C, int dtype, msmc_stream stream);
/* Squeeze-excitation with the block's residual (tdnn.py:122-134, 150-151), x / res / y [B][T][C]:
 *   y = res + x * gate[b],  gate = sigmoid(W2 relu(W1 mean_t(x) + b1) + b2),  W1 [C/2][C], W2 [C][C/2] (nn.Linear layout).
 * C % 8 == 0, C <= 1024, B < 65536.  Forward, three launches: per-slab time sums, one workgroup per batch element (merge + the
 * two matrix-vector products), scale + residual.  gate / mean [B][C] and hidden [B][C/2] (fp32) are kept for the backward. */
size_t msmc_se_workspace(int B, int T, int C);
int msmc_se_fwd(const void* x, const void* res, const float* W1, const float* b1, const float* W2, const float* b2, void* y,
                float* gate, float* mean, float* hidden, void* workspace, size_t workspace_bytes, int B, int T, int C, int dtype,
                msmc_stream stream);
/* Backward over the frames: dgate [B][C] = sum_t g x (per-slab sums, merged in order), and, once the two small layers have been
 * back-propagated on [B][C] quantities, gx = g * gate + dmean with dmean [B][C] the gradient of the time mean divided by T.
 * (The residual's gradient is g itself.) */
int msmc_se_bwd_gate(const void* g, const void* x, float* dgate, void* workspace, size_t workspace_bytes, int B, int T, int C,
                     int dtype, msmc_stream stream);
int msmc_se_bwd_apply(const void* g, const float* gate, const float* dmean, void* gx, int B, int T, int C, int dtype,
                      msmc_stream stream);
/* Attentive statistics pooling (tdnn.py:163-170) of x [B][T][C] under logits a [B][T][C] (the output of linear2):
 *   alpha = softmax_t(a) over all T frames, mean = sum_t alpha x, std = sqrt(max(sum_t alpha x^2 - mean^2, 1e-9)),
 *   out [B][2C] fp32 = (mean | std).  C % 8 == 0, C <= 1536, T >= 1, B < 65536.
 * Forward, two launches: an online softmax per (batch, channel) over splits of T -- x and a are read once -- then the partials
 * (m, l, s1, s2) merged in order.  stats [B][4][C] fp32 = (max, sum of exponentials, mean, residual) is kept for the backward. */
size_t msmc_asp_workspace(int B, int T, int C);
int msmc_asp_fwd(const void* x, const void* a, float* out, float* stats, void* workspace, size_t workspace_bytes, int B, int T,
                 int C, int dtype, msmc_stream stream);
/* Backward, one pass: alpha recomputed from stats; gx and ga [B][T][C] from gout [B][2C] fp32.  Where the clamp is active
 * (residual < 1e-9) no gradient flows through std, as with torch.clamp. */
int msmc_asp_bwd(const float* gout, const void* x, const void* a, const float* stats, void* gx, void* ga, int B, int T, int C,
                 int dtype, msmc_stream stream);

/* ---------------------------------------------------------------------------------------------
 * O1  gradient-norm clipping + AdamW for all tensors of one child in three launches (csrc/optim.hip).
 * Replaces clip_grad_norm_ + the per-child AdamW step of
 *   reference msmctts/trainers/optimizers/__init__.py:53-78, msmctts/trainers/msmctts_trainer.py:205-206.
 * ``table`` is a DEVICE array sorted by first_chunk; tensor i owns workgroups [first_chunk, first_chunk + ceil(n / chunk)).
 * lr [1], step [1] (incremented by the call, as float), norm_coef [2] (out: total gradient norm, clip coefficient) and
 * partial [nblocks] live on the device.  max_norm <= 0: no clipping (coefficient 1).  write_grads != 0: the clipped
 * gradients are written back (clip_grad_norm_'s in-place semantics).  torch.optim.AdamW arithmetic, fp32.
 * ------------------------------------------------------------------------------------------- */
typedef struct msmc_opt_tensor {
    float* p;               /* parameter */
    float* g;               /* gradient */
    float* m;               /* exp_avg */
    float* v;               /* exp_avg_sq */
    long n;                 /* elements */
    int first_chunk;
    int pad_;
} msmc_opt_tensor;
int msmc_opt_chunk(void);   /* elements per workgroup */
int msmc_opt_clip_adamw(const msmc_opt_tensor* table, int ntensors, int nblocks, float max_norm, float* partial,
                        float* norm_coef, const float* lr, float* step, float beta1, float beta2, float eps,
                        float weight_decay, int write_grads, msmc_stream stream);

/* ---------------------------------------------------------------------------------------------
 * A1  acoustic features from waveforms in one launch (csrc/features.hip): normalised log-mel spectrogram and frame energy.
 * Replaces melspectrogram / energy of reference examples/csmsc/scripts/audio/audio.py:23-24, 59-73, 81-85, 95-99, 114-115,
 * 122-129 (pre-emphasis, librosa.stft with center=True, magnitude, Slaney mel, dB, normalise and clip; the l2 norm of the
 * magnitudes per frame).
 *   wav [B][Lmax] fp32, length [B] int32 on the device -> mel [B][Tmax][M] fp32, energy [B][Tmax] fp32 (NULL: not computed).
 *   T_b = 1 + length[b] / hop frames per utterance; rows T_b <= t < Tmax are +0.  Every utterance is reflect-padded by
 *   n_fft / 2 at its OWN length, and its rows do not depend on the rest of the batch or on Lmax.  An utterance whose length
 *   is <= n_fft / 2 (after clamping to [0, Lmax]) is all zeros: the host refuses it before the launch.
 *   basis [ceil(F / FQ)][WP][2 FQ] fp32, F = n_fft / 2 + 1, WP = win rounded up to whole KS: for frequency tile j and tap n the
 *     FQ values w[n] cos(2 pi (n + off) f / n_fft), then the FQ values -w[n] sin(...), f = j FQ .. j FQ + FQ - 1,
 *     off = (n_fft - win) / 2, w the periodic Hann window of win samples; zero for n >= win and f >= F.
 *   melT [ceil(F / FQ) FQ][MP] fp32, MP = M rounded up to whole 32: the mel basis transposed, zero-padded.
 *   FT (frames per workgroup), FQ and KS are what the tile function returns for 0, 1 and 2.
 * Accepted: n_fft even, 1 <= win <= n_fft, hop >= 1, 1 <= M <= 128, Lmax > n_fft / 2, 1 <= B < 65536, Tmax >= 1,
 * min_level_db < 0 < max_abs_value, and a tile's sample span ((FT - 1) min(hop, win) + WP floats) within LDS beside 49.5 KB of
 * other buffers; otherwise MSMC_E_SHAPE and no launch.  Fixed summation orders, no atomics: the same input gives the same bits.
 * ------------------------------------------------------------------------------------------- */
int msmc_mel_features_tile(int which);
int msmc_mel_features(const float* wav, const int* length, const float* basis, const float* melT, float* mel, float* energy,
                      int B, int Lmax, int Tmax, int n_fft, int win, int hop, int M, float preemphasis, float ref_level_db,
                      float min_level_db, float max_abs_value, int symmetric, msmc_stream stream);

/* ---------------------------------------------------------------------------------------------
 * A2  YIN F0 tracks from waveforms in one launch (csrc/pitch.hip), on the frame grid of A1.  No reference counterpart: the
 * reference ships no F0 tracker and fixes only the convention of the track (utils/audio.py lf02sinexi / lf02peakexi: natural-log
 * F0 on voiced frames, a value <= 0 on unvoiced ones).  YIN steps 1-5 (de Cheveigne & Kawahara 2002), no pre-emphasis.
 *   wav [B][Lmax] fp32, length [B] int32 on the device -> pitch [B][Tmax] fp32; optional (NULL: not written) voiced [B][Tmax]
 *   uint8, aperiodicity [B][Tmax] fp32, cmnd [B][Tmax][tau_max + 2] fp32.
 *   T_b = 1 + length[b] / hop frames per utterance; rows T_b <= t < Tmax are zero in every output.  span = W + tau_max + 1.
 *   Frame t: x[j] = y[reflect(t hop - span / 2 + j)], reflected at 0 and at the utterance's OWN length; an utterance whose
 *   length is <= span / 2 (after clamping to [0, Lmax]) is all zeros: the host refuses it before the launch.
 *   d(tau) = sum_{j < W} (x[j] - x[j + tau])^2 for 1 <= tau <= tau_max + 1 (direct form: exactly 0 at the period of a periodic
 *   frame); cmnd[tau] = d'(tau) = d(tau) tau / sum_{k <= tau} d(k) (1 at tau = 0 and where the sum is 0).  The lag is the first
 *   tau in [tau_min, tau_max] with d' < threshold, walked up while d' falls (within tau_max); none: unvoiced.  Parabolic
 *   refinement on d'(lag - 1 .. lag + 1), clipped to one sample; pitch = ln(sample_rate / (lag + delta)), the Hz value with
 *   log_f0 == 0, +0 on unvoiced frames.  aperiodicity = d'(lag), on unvoiced frames the minimum of d' over [tau_min, tau_max].
 *   The tile function returns the frames per workgroup for 0 and the lags a wave holds at a time for 1.
 * Accepted: W, hop, Tmax, sample_rate >= 1, 1 <= B < 65536, 2 <= tau_min < tau_max, threshold > 0, Lmax > span / 2, and
 * ((FT - 1) hop + span + FT ((tau_max + 2) | 1)) floats within 160 KB of LDS; otherwise MSMC_E_SHAPE and no launch.
 * Fixed summation orders (csrc/pitch.hip), no atomics: the same input gives the same bits, whatever the batch.
 * ------------------------------------------------------------------------------------------- */
int msmc_pitch_yin_tile(int which);
int msmc_pitch_yin(const float* wav, const int* length, float* pitch, unsigned char* voiced, float* aperiodicity, float* cmnd,
                   int B, int Lmax, int Tmax, int W, int hop, int tau_min, int tau_max, int sample_rate, float threshold,
                   int log_f0, msmc_stream stream);

/* ---------------------------------------------------------------------------------------------
 * A0  waveform preparation (csrc/resample.hip; host side msmctts_amd/hip/resample.py): downmix, rational resampling and peak
 * normalisation of a padded batch, the step that stands before A1 and A2 (reference examples/csmsc/scripts/audio/
 * audio_normalization.sh: `sox in.wav -c 1 -r $sample_rate --norm=-7 out.wav`).  sox's own filter is not reproduced: the
 * resampler is a Kaiser-windowed-sinc polyphase filter (definition, work mapping and summation order: the source header).
 *   x [B][Lmax_in][C] interleaved, fp32 (x_dtype 0) or int16 (x_dtype 1: scaled by 1 / 32768); length [B] int32 on the device.
 *   The channels of a sample are averaged, (x_0 + ... + x_{C-1}) / C in channel order in fp32 (C == 1: a plain read), then
 *     y[b][n] = sum_{j < P} bank[p][j] xbar[q down + (p down + half) / up - j],  n = q up + p, xbar = 0 outside [0, length[b])
 *   for n < ceil(length[b] up / down); y [B][Lmax_out] fp32 is +0 behind that.  j ascending from +0, fp32, one rounding for the
 *   product and one for the sum.  bank [up][P] fp32: row p holds h[up j + (p down + half) % up - half], h the prototype filter
 *   of 2 half + 1 taps at the up-sampled rate, zero past its end; P == ceil((2 half + 1) / up).
 *   partials [B][msmc_resample_parts(...)] fp32: max |y| of each workgroup's outputs (+0 where it has none), all written.
 *   msmc_resample_tile(which, up, down, P): 0 -> PS, the output phases a workgroup holds, 1 -> QT, the values of q it covers
 *   (so tile borders lie at the multiples of QT up output samples); 0 for a refused shape.
 * Accepted: no NULL operand, x_dtype 0 or 1, 1 <= B < 65536, 1 <= C <= 8, 1 <= up, down <= 1024 and coprime, half >= 0,
 * 1 <= P <= 1024 with P == ceil((2 half + 1) / up), Lmax_in >= 1, Lmax_out >= ceil(Lmax_in up / down), Lmax_out < 2^31 - 2^21;
 * otherwise MSMC_E_SHAPE and no launch.  ONE launch.  An utterance's samples depend neither on its batch nor on Lmax_in nor on
 * what lies behind its length; length[b] is clamped to [0, Lmax_in].
 * ------------------------------------------------------------------------------------------- */
int msmc_resample_tile(int which, int up, int down, int P);
/* the partials per utterance of a call with these shapes; 0 for a refused shape */
int msmc_resample_parts(int Lmax_out, int up, int down, int P);
int msmc_resample(const void* x, int x_dtype, const int* length, const float* bank, float* y, float* partials, int B, int Lmax_in,
                  int C, int Lmax_out, int up, int down, int P, int half, msmc_stream stream);

/* Peak normalisation in place, the second launch: peak_b = max over partials[b][0 .. nparts) (reduced in tile order),
 * gain_b = target / peak_b (one IEEE division), y[b][n] *= gain_b for n < out_length[b] (clamped to [0, Lmax_out]); an utterance
 * whose peak is 0 is left as it is.  peak [B] (may be NULL) receives peak_b.  target = fp32(10^(dB / 20)).
 * Accepted: no NULL operand but peak, 1 <= B < 65536, Lmax_out >= 1, nparts >= 1, target > 0; otherwise MSMC_E_SHAPE, no launch. */
int msmc_peak_scale(float* y, const float* partials, const int* out_length, float* peak, int B, int Lmax_out, int nparts, float target,
                    msmc_stream stream);

/* ---------------------------------------------------------------------------------------------
 * A4  spectrogram and Griffin-Lim (csrc/griffin_lim.hip; host side msmctts_amd/hip/griffin_lim.py), on the frame grid of A1.
 * Replaces spectrogram, inv_preemphasis, _stft / _istft and the loops of _griffin_lim / _fast_griffin_lim of reference
 * examples/csmsc/scripts/audio/audio.py:27-56, 71-78, 176-204 (librosa.stft + librosa.istft per iteration on the CPU).
 *
 * msmc_stft: wav [B][Lmax] fp32, length [B] int32 on the device; T_b = 1 + length[b] / hop frames, reflect-padded by n_fft / 2
 * at the utterance's OWN length, pre-emphasis as in A1 (0: none), basis as in A1; z = re + i im with A1's tap order.
 *   mode 0 (complex): out [B][Tmax][2][F] fp32 -- per frame its F real parts, then its F imaginary parts.  mag, prev NULL.
 *   mode 1 (project): mag [B][Tmax][F] fp32; out (layout of mode 0) = t1 = mag z / |z|, (mag, 0) where z == 0 exactly; within
 *     4 x 2^-24 mag per component of the exact quotient of the fp32 z.  With prev (layout of mode 0, holding t0; NULL: none):
 *     out = t1 + alpha (t1 - t0), prev = t1, each element read and written by one work-item.
 *   mode 2 (db): out [B][Tmax][F] = clip(normalise(20 log10(max(1e-5, |z|)) - ref_level_db)), A1's epilogue per frequency.
 *   Rows T_b <= t < Tmax of out are +0; an utterance with length <= n_fft / 2 is all zero rows.  The tile function returns the
 *   frames per workgroup, the frequencies per tile and the taps per slice for 0, 1, 2 (those of A1), and the samples per carry
 *   step of msmc_deemphasis for 3.
 * Accepted: mode 0..2 with mag exactly in mode 1 and prev only there, n_fft even, 1 <= win <= n_fft, hop >= 1, Lmax > n_fft / 2,
 * 1 <= B < 65536, Tmax >= 1, in mode 2 min_level_db < 0 < max_abs_value, and a tile's sample span within LDS beside 32 KB.
 *
 * msmc_istft: spec [B][Tmax][2][F] fp32 (layout of mode 0), frames [B] int32 on the device (clamped to [0, Tmax]) ->
 * y [B][hop (Tmax - 1)] fp32 = librosa.istft(hop_length, win_length) with its defaults: irfft, periodic Hann window centred in
 * n_fft, overlap-add, division by the summed squared windows where they exceed FLT_MIN, n_fft / 2 trimmed at both ends;
 * samples hop (frames[b] - 1) <= j are +0.
 *   ibasis [ceil(win / 128)][KP][128] fp32, KP = 2 F rounded up to whole 16: for tap tile j and row k the 128 taps n = 128 j ..:
 *     k < F: c_f w[n] cos(2 pi f (n + off) / n_fft) / n_fft, f = k; F <= k < 2 F: -c_f w[n] sin(...) / n_fft, f = k - F, zero for
 *     f = 0 and f = n_fft / 2; c_f = 1 there, 2 otherwise; zero for n >= win and k >= 2 F.  wsq [win] fp32: w[n]^2.
 *   Every sample sums the frames that cover it in ascending t, and the squared windows in the same order; a frame's taps sum
 *   k ascending (real parts, then imaginary parts).  msmc_istft_tile: the frame positions a workgroup owns, 32 - (ceil(win / hop)
 *   - 1); 0 for a refused geometry.
 * Accepted: n_fft even, 1 <= win <= n_fft, hop >= 1, ceil(win / hop) <= 32, (32 win + 5184) floats within 160 KB of LDS
 * (win <= 1118), 1 <= B < 65536, Tmax >= 2, hop (Tmax - 1) + n_fft < 2^31.
 *
 * msmc_deemphasis: y[b][n] = x[b][n] + coef y[b][n - 1] for n < length[b] (clamped to [0, Lmax]), x, y [B][Lmax] fp32, x == y
 * allowed; samples at or behind the length are neither read nor written.  Order: the source header.
 * Accepted: no NULL operand, 1 <= B < 65536, Lmax >= 1.
 *
 * All three: otherwise MSMC_E_SHAPE and no launch; ONE launch each; fixed summation orders, no atomics; an utterance's values
 * depend on its own samples / frames and length only, not on the batch or the padding.
 * ------------------------------------------------------------------------------------------- */
int msmc_stft_tile(int which);
int msmc_stft(const float* wav, const int* length, const float* basis, int mode, float* out, const float* mag, float* prev,
              float alpha, int B, int Lmax, int Tmax, int n_fft, int win, int hop, float preemphasis, float ref_level_db,
              float min_level_db, float max_abs_value, int symmetric, msmc_stream stream);
int msmc_istft_tile(int n_fft, int win, int hop);
int msmc_istft(const float* spec, const int* frames, const float* ibasis, const float* wsq, float* y, int B, int Tmax, int n_fft,
               int win, int hop, msmc_stream stream);
int msmc_deemphasis(const float* x, float* y, const int* length, int B, int Lmax, float coef, msmc_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* MSMC_HIP_H */
