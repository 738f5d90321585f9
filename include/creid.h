/*
 * creid.h -- C ABI of libcreid_hip.so: the MI355X (gfx950) implementation of the
 * centroids-reid embedding-and-retrieval hot path.
 *
 * The upstream project (mikwieczorek/centroids-reid) is pure Python and has no FFI layer;
 * its boundary for this path is the Python object surface listed in SURVEY.md section 8b.
 * Each entry point below names the reference function (file:line, relative to the
 * upstream repository root) whose arithmetic it replaces; the Python mirror of that
 * surface (package `centroids-reid_amd`) binds these symbols with ctypes
 * (see INTEGRATION.md for the binding a maintainer would add upstream).
 *
 * Conventions (all functions):
 *   - every pointer is a DEVICE pointer borrowed from the caller (torch owns all memory);
 *     the library allocates nothing; scratch comes in through `ws` + `*_workspace_bytes()`;
 *   - sizes / leading dimensions are int64_t element counts, row-major;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream);
 *   - returns 0 on success, <0 for an argument error (CREID_E_*), >0 = hipError_t of the
 *     launch; never throws, never synchronises the stream, re-entrant.  Process-global state is limited to immutable
 *     kernel handles / zero pages and the optional launch-plan registry (creid_tune_set / creid_tune_clear below: host-side,
 *     written before the first launch, read-only afterwards).
 */
#ifndef CREID_H
#define CREID_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CREID_ABI_VERSION 1

/* CREID_BF16X3 is a convolution mode, not a storage type: fp32 activations in and out, weights pre-split into two bf16 planes
 * (hi = bf16(w), lo = bf16(w - hi)), and every product expanded into three bf16 MFMAs (lo*hi + hi*lo + hi*hi, fp32
 * accumulation) -- fp32-grade results from the bf16 matrix pipe.  It is accepted ONLY by creid_conv2d_fwd_nhwc,
 * creid_conv2d_fwd_affine_nhwc, creid_weight_prep and creid_weight_prep_multi; every other entry point that takes a dtype
 * returns CREID_E_DTYPE for it (the rest of the eval forward runs with CREID_F32 on the fp32 activations).  Training in the mode
 * uses entry points of its own, which take no dtype: creid_conv2d_dgrad_x3_nhwc, creid_conv2d_wgrad_x3_nhwc / _partials and
 * creid_weight_prep_x3_train_multi (every other launch of a training step runs with CREID_F32). */
enum { CREID_F32 = 0, CREID_BF16 = 1, CREID_F16 = 2, CREID_BF16X3 = 3 };
enum { CREID_E_ARG = -1, CREID_E_DTYPE = -2, CREID_E_WS = -3, CREID_E_SHAPE = -4 };

int creid_abi_version(void);

/* ------------------------------------------------------------------ stage D: distance */

/* utils/reid_metric.py:113-115 (F.normalize p=2 dim=1): y[r,:] = x[r,:] / max(||x[r]||, eps).
 * x fp32 [rows, D]; y has dtype `out_dtype` (CREID_F32 / CREID_BF16 / CREID_F16);
 * sqnorm (nullable) receives sum_k y[r,k]^2 accumulated in fp32 from the ROUNDED y. D % 4 == 0. */
int creid_l2norm_rows(const float* x, void* y, float* sqnorm, int64_t rows, int64_t D,
                      int out_dtype, float eps, void* stream);

/* torch.pow(x,2).sum(dim=1) of utils/reid_metric.py:28-30 / losses/triplet_loss.py:35-36. */
int creid_row_sqnorm(const void* x, float* out, int64_t rows, int64_t D, int dtype, void* stream);

/* utils/reid_metric.py:25-33 get_euclidean: out[i,j] = (qq[i] + gg[j]) - 2 * <q_i, g_j>
 * (squared L2, no clamp, no sqrt).  q [m,D], g [n,D] of `dtype`; qq [m], gg [n] fp32 row
 * square-norms; out fp32 [m, ldo].  fp32 inputs run on v_mfma_f32_32x32x2_f32 (exact f32
 * FMA chain); bf16/f16 inputs on v_mfma_f32_32x32x16_{bf16,f16} with fp32 accumulate. */
int creid_sqdist_matrix(const void* q, const void* g, const float* qq, const float* gg,
                        int64_t m, int64_t n, int64_t D, int dtype, float* out, int64_t ldo,
                        void* stream);

/* ------------------------------------------------------------------ stage D/E: rank */

/* utils/reid_metric.py:129,132 np.argsort(distmat, axis=1): per-row ascending order of
 * (distance, gallery index) -- ties broken by index (the reference leaves ties undefined).
 * dist fp32 [m, ld]; out_idx int64 [m, n]. */
size_t creid_rank_rows_workspace_bytes(int64_t m, int64_t n);
int creid_rank_rows(const float* dist, int64_t m, int64_t n, int64_t ld, int64_t* out_idx,
                    void* ws, size_t ws_bytes, void* stream);
/* np.argsort + eval_func's per-query loop (utils/reid_metric.py:129-132 + utils/eval_reid.py:36-90, plain camera ids) in ONE
 * pass: the ranked row is evaluated while it is still in LDS, so the int64 index matrix (8 B per pair) is written for the
 * caller but never read back; rows the one-pass rank kernel cannot take are evaluated by creid_cmc_ap_ranked's kernel.
 * out_idx / ws as creid_rank_rows, out_valid / out_ap / out_first as creid_cmc_ap_ranked; results identical to the two calls. */
int creid_rank_rows_eval(const float* dist, int64_t m, int64_t n, int64_t ld, int64_t* out_idx, void* ws, size_t ws_bytes,
                         const int64_t* q_pids, const int64_t* g_pids, const int64_t* q_camids, const int64_t* g_camids,
                         uint8_t* out_valid, double* out_ap, int32_t* out_first, void* stream);

/* ------------------------------------------------------------------ stage E: CMC / mAP */

/* utils/eval_reid.py:44-84 (the per-query loop of eval_func, respect_camids=False), one
 * workgroup per query over the ranked row: drop gallery entries with the query's pid AND
 * camid (:57); valid = any match left (:63-65); ap = sum_k [match_k] * cum_k / (k+1) / n_rel
 * in float64 (:75-79); first = 0-based kept-rank of the first match (defines the clipped
 * CMC row :67-70 and the top-k flags :18-22).  idx int64 [m, n]; pids/camids int64. */
int creid_cmc_ap_ranked(const int64_t* idx, int64_t m, int64_t n, const int64_t* q_pids,
                        const int64_t* g_pids, const int64_t* q_camids, const int64_t* g_camids,
                        uint8_t* out_valid, double* out_ap, int32_t* out_first, void* stream);

/* The same scan for camera-set gallery entries (respect_camids=True, utils/eval_reid.py:51-55, fed by
 * modelling/bases.py:205-236): g_cam_masks[j] = bitmask of the camera ids (< 64) of gallery entry j; an entry
 * is dropped for a query iff it has the query's pid AND bit q_camids[i] is set in its mask. */
int creid_cmc_ap_ranked_camsets(const int64_t* idx, int64_t m, int64_t n, const int64_t* q_pids,
                                const int64_t* g_pids, const int64_t* q_camids, const int64_t* g_cam_masks,
                                uint8_t* out_valid, double* out_ap, int32_t* out_first, void* stream);

/* The k smallest (distance, index) pairs of every row of dist fp32 [m, ld >= n], ascending -- what
 * inference/get_similar.py:114-119 keeps of its full argsort (`indices[:, :topk]`) -- without ranking the rest.
 * k <= min(n, 1024).  out_idx int64 [m][k]; out_dist fp32 [m][k] (nullable) the corresponding distances; ties resolve by
 * index like creid_rank_rows.  flags uint8 [m]: 1 = the row's candidate set did not fit (massive ties at the k-th
 * distance): that row's outputs are unwritten, use creid_rank_rows for it. */
int creid_topk_rows(const float* dist, int64_t m, int64_t n, int64_t ld, int32_t k, int64_t* out_idx,
                    float* out_dist, uint8_t* flags, void* stream);

/* utils/eval_reid.py:86-90: means over valid queries.  out_cmc float32[max_rank]
 * (= count(first<=r)/n_valid in float32), out_map float64[1], out_topk float64[5] for
 * k in {1,5,10,20,50}, out_nvalid int64[1]. */
int creid_eval_reduce(const uint8_t* valid, const double* ap, const int32_t* first, int64_t m,
                      int32_t max_rank, float* out_cmc, double* out_map, double* out_topk,
                      int64_t* out_nvalid, void* stream);


/* ---- metric-only evaluation with NO m x n matrix (csrc/stream_eval.hip): what utils/reid_metric.py:93-151 +
 * utils/eval_reid.py:25-92 compute, for plain camera ids and the squared-L2 distance.  Three launches:
 *  poslist : per query, distances to its positives (gallery rows of the same pid, other camera) in the arithmetic
 *            of creid_sqdist_matrix, sorted by (distance, gallery index).  The gallery is given grouped by pid:
 *            g_order int32 [n] (gallery indices grouped by pid; any order inside a group -- the kernel re-ranks its
 *            candidates by (distance, gallery index)), csr_off int64 [n_groups + 1], q_slot int32 [m] (the query
 *            pid's group, -1 if absent) -- built on the device by creid_stream_plan.  cap = list capacity per query
 *            (power of two, 2..128); pos_key uint32 [m][cap] (order-preserving image of the fp32 distance, padded
 *            with 0xffffffff), pos_idx int32 [m][cap], npos int32 [m] (-1: more than cap positives -- such queries
 *            must take creid_sqdist_matrix + creid_rank_rows + creid_cmc_ap_ranked instead).
 *  count   : the full contraction, tile by tile on the f32 MFMA pipe; every negative (other pid) bumps
 *            hist[q][#positives ranked before it] -- hist uint32 [m][cap] must be ZERO on entry.
 *  finalize: valid uint8 [m] (0: no positive, 1: ok, 2: overflow), ap float64 [m], first int32 [m] with the
 *            meaning of creid_cmc_ap_ranked; feed creid_eval_reduce. */
/* The index of the three launches above, built on the device from the raw label vectors (the per-query `matches` /
 * `remove` bookkeeping of utils/eval_reid.py:36-65 done once for all queries): counting sort of the gallery by pid over the
 * dense range [pmin, pmin + R) (R = max pid - min pid + 1 of the gallery; group = pid - pmin), then per query its group,
 * its number of positives n_pos (same pid, other camera) and stats int32[2] = {max n_pos over queries with n_pos <= 128,
 * number of queries with more}.  csr_off int64[R + 1], g_order int32[n], q_slot / n_pos int32[m], scratch int32[2 R].
 * No host synchronisation; the caller reads `stats` (8 bytes) to choose cap. */
int creid_stream_plan(const int64_t* q_pids, const int64_t* g_pids, const int64_t* q_cams, const int64_t* g_cams,
                      int64_t m, int64_t n, int64_t pmin, int64_t R, int64_t* csr_off, int32_t* g_order,
                      int32_t* q_slot, int32_t* n_pos, int32_t* stats, int32_t* scratch, void* stream);
int creid_stream_poslist(const float* q, const float* g, const float* qq, const float* gg, int64_t m, int64_t n,
                         int64_t D, const int32_t* q_slot, const int64_t* csr_off, const int32_t* g_order,
                         const int64_t* q_cams, const int64_t* g_cams, int32_t cap, uint32_t* pos_key,
                         int32_t* pos_idx, int32_t* npos, void* stream);
int creid_stream_count(const float* q, const float* g, const float* qq, const float* gg, int64_t m, int64_t n,
                       int64_t D, const int64_t* q_pids, const int64_t* g_pids, int32_t cap,
                       const uint32_t* pos_key, const int32_t* pos_idx, const int32_t* npos, uint32_t* hist,
                       void* stream);
int creid_stream_finalize(const int32_t* npos, const uint32_t* hist, int64_t m, int32_t cap, uint8_t* valid,
                          double* ap, int32_t* first, void* stream);

/* The streamed evaluation for gallery entries that carry camera SETS (respect_camids=True: the camera-aware centroids of
 * modelling/bases.py:205-236, or any gallery of camera sets): g_cam_masks int64 [n], bit c set = camera c in the entry's
 * set; q_cams plain camera ids, which the CALLER keeps inside 0..62 (the kernels shift a 64-bit mask by them).  A same-pid
 * entry is removed for a query iff the query's camera is in its set (utils/eval_reid.py:51-55, the test of
 * creid_cmc_ap_ranked_camsets); everything else -- arguments, limits, outputs -- is creid_stream_plan / creid_stream_poslist.
 * Camera sets only change which same-pid entries are positives, so creid_stream_count and creid_stream_finalize (and
 * creid_stream_count_h16) serve both forms unchanged. */
int creid_stream_plan_camsets(const int64_t* q_pids, const int64_t* g_pids, const int64_t* q_cams,
                              const int64_t* g_cam_masks, int64_t m, int64_t n, int64_t pmin, int64_t R, int64_t* csr_off,
                              int32_t* g_order, int32_t* q_slot, int32_t* n_pos, int32_t* stats, int32_t* scratch,
                              void* stream);
int creid_stream_poslist_camsets(const float* q, const float* g, const float* qq, const float* gg, int64_t m, int64_t n,
                                 int64_t D, const int32_t* q_slot, const int64_t* csr_off, const int32_t* g_order,
                                 const int64_t* q_cams, const int64_t* g_cam_masks, int32_t cap, uint32_t* pos_key,
                                 int32_t* pos_idx, int32_t* npos, void* stream);

/* ---- camera-aware centroid index on the device (csrc/centroid_index.hip): the grouping loop of modelling/bases.py:205-236.
 * labels int64 [2][num_query + num_gallery] on the device: row 0 the pids, row 1 the camera ids, queries first.  The camera of
 * gallery row j is labels[1][j] (the reference indexes the full vector with the gallery-relative index, :214 -- kept), a
 * query's is labels[1][i]; the CALLER keeps labels[1][0 .. max(num_query, num_gallery)) inside 0..62.  [pmin, pmin + R) must
 * cover every gallery pid.  Per gallery pid (ascending) that has a query, with gmask / qmask the OR of its rows' / queries'
 * cameras, for cur over the bits of qmask (ascending): cur in gmask -> one centroid of the rows whose camera is not cur, with
 * set gmask & ~(1 << cur), nothing when that set is empty; cur not in gmask -> the first such cur gives one centroid of all
 * the pid's rows with set gmask, later ones nothing.
 *  ws_bytes: size of the workspace `ws` (0 for an empty gallery or range).
 *  plan    : counting sort + sizes; totals int64 [2] on the device = {n_cent, rows}: the one read-back, which sizes:
 *  fill    : order int64 [rows] (full-vector row numbers = gallery index + num_query, ascending inside a centroid: the order
 *            creid_gather_mean_rows sums in), offsets int64 [n_cent + 1], cent_labels int64 [n_cent] (the pid), cent_masks
 *            int64 [n_cent] (bit c = camera c).  ws, labels and the sizes as given to / read from `plan`.
 * Integer atomics only: the arrays do not depend on the run.  CREID_E_SHAPE when num_query + num_gallery >= 2^31 - 16 or
 * R > 2^26. */
size_t creid_centroid_index_ws_bytes(int64_t num_gallery, int64_t R);
int creid_centroid_index_plan(const int64_t* labels, int64_t num_query, int64_t num_gallery, int64_t pmin, int64_t R,
                              void* ws, int64_t* totals, void* stream);
int creid_centroid_index_fill(const int64_t* labels, int64_t num_query, int64_t num_gallery, int64_t pmin, int64_t R,
                              const void* ws, int64_t n_cent, int64_t rows, int64_t* order, int64_t* offsets,
                              int64_t* cent_labels, int64_t* cent_masks, void* stream);

/* ---- top-k retrieval with NO m x n matrix (csrc/stream_eval.hip): what creid_sqdist_matrix (fp32) + creid_topk_rows
 * return -- the same indices and the same distance bits, ties by gallery index -- from the streamed contraction.
 *  collect : q fp32 [m][D], g fp32 [n][D], qq / gg their row square norms, D % 4 == 0.  tau fp32 [m]: ANY upper bound
 *            (inclusive) on the row's k-th smallest distance, e.g. the k-th smallest over a sample of >= k gallery rows
 *            computed by creid_sqdist_matrix.  Every column with distance <= tau[row] takes a slot of the row's list:
 *            count int32 [m] (must be ZERO on entry) ends as the number of such columns, cand uint64 [m][cap] holds the
 *            first min(count, cap) of them in arrival order as (order-preserving image of the fp32 distance) << 32 | column.
 *            cap = a power of two, 64..8192.
 *  select  : per row the k smallest (distance, index) of its list, ascending: out_idx int64 [m][k], out_dist fp32 [m][k]
 *            (nullable).  k <= min(1024, cap).  flags uint8 [m]: 0 = written; 1 = the list overflowed (count > cap) or
 *            holds fewer than k entries (NaN distances pass no threshold): that row's outputs are unwritten, use
 *            creid_sqdist_matrix + creid_topk_rows for it.
 * CREID_E_SHAPE for a cap / k / D outside these limits, before anything is launched; m == 0 returns 0. */
int creid_stream_topk_collect(const float* q, const float* g, const float* qq, const float* gg, int64_t m, int64_t n,
                              int64_t D, const float* tau, int32_t cap, uint64_t* cand, int32_t* count, void* stream);
int creid_stream_topk_select(const uint64_t* cand, const int32_t* count, int64_t m, int32_t cap, int32_t k,
                             int64_t* out_idx, float* out_dist, uint8_t* flags, void* stream);

/* ---- the streamed evaluation and the streamed retrieval for 16-bit features (csrc/stream_h16.hip): q / g are bf16 or f16
 * [m][D] / [n][D] (dtype = CREID_BF16 | CREID_F16, both operands alike), qq / gg their fp32 row square norms; every other
 * argument has the meaning, the limits and the checks of the fp32 entry point of the same name without _h16 (cap rules, size
 * limits, m == 0 returns 0 before the pointer checks), plus D % 8 == 0 (16-byte k-chunks; D <= 2^20) else CREID_E_SHAPE and
 * any other dtype CREID_E_DTYPE -- all before anything is launched.  creid_stream_plan, creid_stream_finalize and
 * creid_stream_topk_select do not depend on the feature type and serve both.
 * Contract: a distance is produced with the bits of creid_sqdist_matrix of the SAME dtype -- every accumulator element
 * starts at 0 and receives one v_mfma_f32_32x32x16_{bf16,f16} per 16-deep k-step in ascending k, lane (l31, kh) supplying
 * k = 16 step + 8 kh + 0..7 in fragment elements 0..7, k beyond D zero-filled in 16-byte chunks, the query as the A operand;
 * distance = fmaf(-2, acc, qq[row] + gg[col]).  poslist computes its <= 128 distances per query with the same instruction in
 * the same step order (the internal summation of a 16-bit MFMA has no scalar equivalent).  Hence the streamed results equal
 * creid_sqdist_matrix + creid_rank_rows + creid_cmc_ap_ranked / creid_topk_rows on the same 16-bit tensors bit for bit. */
int creid_stream_poslist_h16(const void* q, const void* g, const float* qq, const float* gg, int64_t m, int64_t n,
                             int64_t D, int dtype, const int32_t* q_slot, const int64_t* csr_off, const int32_t* g_order,
                             const int64_t* q_cams, const int64_t* g_cams, int32_t cap, uint32_t* pos_key,
                             int32_t* pos_idx, int32_t* npos, void* stream);
/* (camera-set gallery entries: see creid_stream_poslist_camsets) */
int creid_stream_poslist_h16_camsets(const void* q, const void* g, const float* qq, const float* gg, int64_t m, int64_t n,
                                     int64_t D, int dtype, const int32_t* q_slot, const int64_t* csr_off,
                                     const int32_t* g_order, const int64_t* q_cams, const int64_t* g_cam_masks, int32_t cap,
                                     uint32_t* pos_key, int32_t* pos_idx, int32_t* npos, void* stream);
int creid_stream_count_h16(const void* q, const void* g, const float* qq, const float* gg, int64_t m, int64_t n,
                           int64_t D, int dtype, const int64_t* q_pids, const int64_t* g_pids, int32_t cap,
                           const uint32_t* pos_key, const int32_t* pos_idx, const int32_t* npos, uint32_t* hist,
                           void* stream);
int creid_stream_topk_collect_h16(const void* q, const void* g, const float* qq, const float* gg, int64_t m, int64_t n,
                                  int64_t D, int dtype, const float* tau, int32_t cap, uint64_t* cand, int32_t* count,
                                  void* stream);

/* ---- ranked lists under the evaluation protocol, with NO m x n matrix: the first k gallery entries of a query that are not
 * junk (utils/eval_reid.py:49-58, the lists utils/visrank.py:193-232 draws).  Entry j is junk for query i when
 * g_pids[j] == q_pids[i] and -- camsets == 0 -- g_cams[j] == q_cams[i], or -- camsets != 0 -- bit q_cams[i] of the camera-set
 * mask g_cams[j] is set (q_cams inside 0..62: the CALLER checks, as for creid_stream_plan_camsets).  All four int64, on the
 * device.
 *  collect_keep / collect_keep_h16: creid_stream_topk_collect / _h16 -- same arguments, limits, checks and distance bits --
 *            where a column takes a slot only if it is not junk.  tau must bound the k-th smallest distance over the row's
 *            NON-junk columns.  creid_stream_topk_select then serves unchanged: a row with fewer than k entries is flagged.
 *  creid_rank_keep_topk: the materialised form.  idx int64 [m][n]: ranked gallery indices (creid_rank_rows); ng: the length
 *            of g_pids / g_cams (an index outside [0, ng) is dropped).  out_idx int64 [m][k]: the first k non-junk entries of
 *            each row in order, padded with -1; out_matched uint8 [m][k]: g_pids[out_idx] == q_pids[row], 0 in the padding;
 *            out_count int32 [m]: the entries that are real.  1 <= k <= 1024 else CREID_E_SHAPE; m == 0 returns 0.
 *  creid_junk_mask_rows: dist fp32 [m][ld >= n], column j = entry j of g_pids / g_cams: junk cells become +inf, in place (the
 *            threshold sample of the streamed form). */
int creid_stream_topk_collect_keep(const float* q, const float* g, const float* qq, const float* gg, int64_t m, int64_t n,
                                   int64_t D, const float* tau, const int64_t* q_pids, const int64_t* g_pids,
                                   const int64_t* q_cams, const int64_t* g_cams, int32_t camsets, int32_t cap, uint64_t* cand,
                                   int32_t* count, void* stream);
int creid_stream_topk_collect_keep_h16(const void* q, const void* g, const float* qq, const float* gg, int64_t m, int64_t n,
                                       int64_t D, int dtype, const float* tau, const int64_t* q_pids, const int64_t* g_pids,
                                       const int64_t* q_cams, const int64_t* g_cams, int32_t camsets, int32_t cap,
                                       uint64_t* cand, int32_t* count, void* stream);
int creid_rank_keep_topk(const int64_t* idx, int64_t m, int64_t n, int64_t ng, int32_t k, const int64_t* q_pids,
                         const int64_t* g_pids, const int64_t* q_cams, const int64_t* g_cams, int32_t camsets,
                         int64_t* out_idx, uint8_t* out_matched, int32_t* out_count, void* stream);
int creid_junk_mask_rows(float* dist, int64_t m, int64_t n, int64_t ld, const int64_t* q_pids, const int64_t* g_pids,
                         const int64_t* q_cams, const int64_t* g_cams, int32_t camsets, void* stream);

/* ---- open-set operating points (TAR @ FAR) with NO m x n matrix (csrc/stream_consume.hpp EPI_HIST, csrc/roc.hip): a radix
 * select over key(i, j), the order-preserving 32-bit key of the distance (sign bit set: key = bits ^ 0xffffffff, else
 * bits ^ 0x80000000).  Pair (i, j) is junk as for the ranked lists above (q_pids / g_pids / q_cams / g_cams / camsets: the same
 * arrays and the same caller-side camera check) and counts nowhere; else it is genuine (class 0: the same pid) or an impostor
 * (class 1: another pid).
 *  hist passes: hist uint64 [nsel][2][2^bits]; for selector s a non-junk pair counts when prefix_bits == 0 or
 *            key >> (32 - prefix_bits) == prefix[s] (uint32 [nsel] on the device; may be NULL without prefix bits), in bin
 *            (key >> (32 - prefix_bits - bits)) & (2^bits - 1) of hist[s][class].  The call ADDS into hist: the caller zeroes
 *            it, and calls over chunks of the queries accumulate.  Integer atomics only: the counts depend on nothing but the
 *            keys.  1 <= bits <= 11, prefix_bits + bits <= 32, 1 <= nsel, nsel << bits <= 8192, nsel == 1 without prefix bits,
 *            else CREID_E_SHAPE.  NaN distances are counted under whatever key their bits give.
 *            creid_stream_dist_hist / _h16: the keys of the distances creid_stream_count / _h16 forms from the same rows
 *            (the bits of creid_sqdist_matrix of the same dtype), with those entry points' limits on D, m, n and dtype; every
 *            refusal of a shape or dtype comes first, then m == 0 returns 0, then the pointer checks.
 *            creid_dist_hist_matrix: the keys of an existing dense fp32 matrix dist [m][n].
 *  creid_roc_descend: the select step after a pass, one workgroup per target t < nsel (the first pass, level == 0, has one
 *            selector that every target reads; later passes selector t).  state int64 [nsel][8] = { rank left inside the
 *            prefix, prefix, impostors below, genuines below, N_imp, N_gen, lowest key of the prefix, flags }.  level == 0
 *            initialises it: N_imp / N_gen = the class totals, rank k = min(floor(far[t] * N_imp), N_imp - 1) (far float64
 *            [nsel] on the device; the one floating-point operation).  Every level walks the impostor counts to the digit that
 *            holds the rank, adds the counts of both classes below it, appends the digit to the prefix and writes prefix[t]
 *            for the next pass.  Once the passes' bits add up to 32 the key slot is the impostor key of 0-based rank k, and
 *            the two counts are the impostor / genuine keys STRICTLY below it.  flags bit 0: N_imp == 0; bit 1: the counts do
 *            not hold the rank (hist is not this state's pass); bits 8..15: the key bits fixed so far.  No host
 *            synchronisation. */
int creid_stream_dist_hist(const float* q, const float* g, const float* qq, const float* gg, int64_t m, int64_t n, int64_t D,
                           const int64_t* q_pids, const int64_t* g_pids, const int64_t* q_cams, const int64_t* g_cams,
                           int32_t camsets, const uint32_t* prefix, int32_t nsel, int32_t prefix_bits, int32_t bits,
                           uint64_t* hist, void* stream);
int creid_stream_dist_hist_h16(const void* q, const void* g, const float* qq, const float* gg, int64_t m, int64_t n,
                               int64_t D, int dtype, const int64_t* q_pids, const int64_t* g_pids, const int64_t* q_cams,
                               const int64_t* g_cams, int32_t camsets, const uint32_t* prefix, int32_t nsel,
                               int32_t prefix_bits, int32_t bits, uint64_t* hist, void* stream);
int creid_dist_hist_matrix(const float* dist, int64_t m, int64_t n, const int64_t* q_pids, const int64_t* g_pids,
                           const int64_t* q_cams, const int64_t* g_cams, int32_t camsets, const uint32_t* prefix,
                           int32_t nsel, int32_t prefix_bits, int32_t bits, uint64_t* hist, void* stream);
int creid_roc_descend(const uint64_t* hist, int32_t nsel, int32_t bits, int32_t level, const double* far, int64_t* state,
                      uint32_t* prefix, void* stream);

/* ---- exact fp32 top-k with the contraction on the 16-bit MFMA (csrc/stream_prefilter.hip): the 16-bit streamed contraction
 * only pre-filters, with a proven margin; the pairs it keeps are re-scored with the fp32 kernels' arithmetic, so the result has
 * the indices and the distance bits of creid_stream_topk_collect + creid_stream_topk_select on the fp32 rows.
 *  pack    : x fp32 [rows][D] -> y = x rounded once to dtype (CREID_BF16 | CREID_F16, round to nearest even; else
 *            CREID_E_DTYPE) and stats float64 [rows][3] = { |x - y|^2, |y|^2, |x|^2 } per row, accumulated in double; a row
 *            with an Inf / NaN element or one that overflows f16 has non-finite statistics.  D % 8 == 0, D <= 2^20, else
 *            CREID_E_SHAPE; rows == 0 returns 0.
 *  (collect: creid_stream_topk_collect_h16 on the packed rows with the FP32 rows' qq / gg and tau[i] >= dh_(k) + 2 m_i, where
 *            dh_(k) is the row's k-th smallest 16-bit distance and m_i >= |16-bit distance - fp32 distance| over the row.)
 *  rescore : in place of creid_stream_topk_select.  cand / count / cap / k / out_idx / out_dist as there; q fp32 [m][D],
 *            g fp32 [n][D], qq / gg as given to the collect; margin2 fp32 [m] >= 2 m_i, rounded up by the caller.  Per row: the
 *            entries with 16-bit distance <= (the list's k-th smallest + margin2[row], rounded up) are kept, each receives the
 *            fp32 distance fmaf(-2, <q_i, g_j> as the k-ordered fmaf chain from zero, qq[i] + gg[j]) -- the bits of
 *            creid_sqdist_matrix on fp32 -- and the k smallest (distance, index) are written.  kept int32 [m]: the number of
 *            kept entries.  flags uint8 [m]: 0 = written; 1 = unwritten, use creid_sqdist_matrix + creid_topk_rows on the fp32
 *            rows: the list overflowed or holds fewer than k entries, margin2[row] is not a finite number >= 0, more than 1024
 *            entries (the re-score capacity) are kept, or a listed column is >= n.  D % 4 == 0, D <= 2^20, cap and k as for
 *            select, else CREID_E_SHAPE; m == 0 returns 0.
 * Every check happens before anything is launched. */
int creid_prefilter_pack(const float* x, int64_t rows, int64_t D, int dtype, void* y, double* stats, void* stream);
int creid_stream_topk_rescore(const uint64_t* cand, const int32_t* count, int64_t m, int32_t cap, int32_t k,
                              const float* q, const float* g, const float* qq, const float* gg, int64_t n, int64_t D,
                              const float* margin2, int64_t* out_idx, float* out_dist, uint8_t* flags, int32_t* kept,
                              void* stream);

/* ---- exact fp32 CMC / mAP with the counting contraction on the 16-bit MFMA (csrc/stream_h16.hip, csrc/stream_prefilter.hip): in
 * place of creid_stream_count on the fp32 rows.  hist ends as creid_stream_count's, element for element, for every row that is not
 * flagged; creid_stream_plan, creid_stream_poslist (on the FP32 rows) and creid_stream_finalize are unchanged.
 *  band    : q / g the rows rounded once to dtype (creid_prefilter_pack), qq / gg the FP32 rows' norms, so that only the dot product
 *            differs from the fp32 distance d; margin fp32 [m]: m_i >= |16-bit distance dh - d| over row i, rounded up by the
 *            caller; pos_key / pos_idx / npos: creid_stream_poslist's lists of the fp32 rows; everything else as
 *            creid_stream_count_h16.  Per negative j of query i (same-pid columns are skipped), with lo = dh - m_i moved one fp32
 *            step down and hi = dh + m_i moved one step up: key(lo) above the row's last positive key -- behind every positive,
 *            nothing to count; else l = the number of positives with key < key(lo), each ranked before j whatever d is; if
 *            l < npos and pos_key[l] <= key(hi), a positive lies inside the band: the pair is ambiguous, amb_count[i] is bumped
 *            and, while the slot is below amb_cap, the column is stored in amb uint32 [m][amb_cap] (arrival order); otherwise
 *            hist[i][l] is bumped, the slot the fp32 kernel finds.  A pair whose dh, lo or hi is not finite is ambiguous.
 *            amb_cap = a power of two, 64..8192.  amb_count int32 [m] and hist must be ZERO on entry.
 *  rescore : every listed pair receives the fp32 distance fmaf(-2, <q_i, g_j> as the k-ordered fmaf chain from zero,
 *            qq[i] + gg[j]) -- the bits of creid_sqdist_matrix on fp32 -- and goes through creid_stream_count's search (ties
 *            with a positive by gallery index): hist[i][l] += 1 when it ranks before a positive.  q fp32 [m][D], g fp32 [n][D],
 *            D % 4 == 0, D <= 2^20.  flags uint8 [m]: 0 = the row's hist is complete; 1 = nothing was added for the row, use
 *            creid_stream_count on the fp32 row with a zeroed hist: amb_count[i] > amb_cap or a listed column is >= n.
 * CREID_E_SHAPE / CREID_E_DTYPE for a cap, amb_cap, D or dtype outside these limits; every check happens before anything is
 * launched; m == 0 returns 0. */
int creid_stream_count_band_h16(const void* q, const void* g, const float* qq, const float* gg, int64_t m, int64_t n,
                                int64_t D, int dtype, const int64_t* q_pids, const int64_t* g_pids, int32_t cap,
                                const uint32_t* pos_key, const int32_t* pos_idx, const int32_t* npos, const float* margin,
                                int32_t amb_cap, uint32_t* amb, int32_t* amb_count, uint32_t* hist, void* stream);
int creid_stream_count_rescore(const uint32_t* amb, const int32_t* amb_count, int64_t m, int32_t amb_cap, const float* q,
                               const float* g, const float* qq, const float* gg, int64_t n, int64_t D, int32_t cap,
                               const uint32_t* pos_key, const int32_t* pos_idx, const int32_t* npos, uint32_t* hist,
                               uint8_t* flags, void* stream);

/* ---- k-reciprocal re-ranking (Zhong et al., CVPR 2017; csrc/rerank.hip): the sparse stages between the streamed top-k and
 * the ranking kernels.  X = cat(q, g) fp32 [N][D], d = creid_sqdist_matrix's squared L2, every ordering by (d, index);
 * nb int64 [N][K], K = k1 + 1: row i's K nearest columns of X (creid_stream_topk_* on (X, X)); rowmax fp32 [N]:
 * M_i = max_j d(i, j); od(i, j) = d(i, j) / M_i (0 where M_i == 0).  Sparse rows are CSR: rowptr int64 [N + 1], columns
 * int32 ascending and distinct inside a row, values fp32.
 *  recip   : R(i, k) = { j in nb[i][:k+1] : i in nb[j][:k+1] };  R*(i) = R(i, k1) united with every R(c, kh), c in R(i, k1),
 *            that has 3 |R(c, kh) & R(i, k1)| > 2 |R(c, kh)|.  cols == NULL: count int32 [N] receives |R*(i)|; else
 *            cols[rowptr[i] ..] receives R*(i) (rowptr = the exclusive scan of count).  0 <= kh < K <= min(N, 1024);
 *            CREID_E_SHAPE when a worst-case row, K (kh + 2) entries, does not fit the kernel's LDS.
 *  weights : vals[p] = exp(-od(i, j)) / sum over row i of exp(-od(i, .)) for every listed (i, j = cols[p]), with
 *            d(i, j) = fmaf(-2, <x_i, x_j>, qq[i] + qq[j]); qq fp32 [N] the row square norms; D % 4 == 0, D <= 16380.
 *  expand  : V'(i) = (1 / k2) sum_{t < k2} V(nb[i][t]), addends in that order.  cap = a power of two >= the largest
 *            sum_{t < k2} |V(nb[i][t])| over all rows (12 cap + 4 k2 bytes of LDS must fit, else CREID_E_SHAPE).
 *            cols2 == NULL: count2 int32 [N] receives |V'(i)|; else cols2 / vals2 [rowptr2[i] ..] receive the row.
 *  blend   : out[i][j] = (1 - lambda) J(i, nq + j) + lambda dist[i][j] / M_i over dist fp32 [nq][ng] =
 *            creid_sqdist_matrix(q, g), J = 1 - s / (2 - s), s = sum_c min(V'(i, c), V'(nq + j, c)) in ascending c.  A dense
 *            pass writes (1 - lambda) + lambda dist / M_i (J = 1: no shared column) everywhere; a sparse pass rewrites the
 *            pairs that share a column, found through colptr int64 [N + 1] / colrows int32: the gallery rows of V' (row
 *            indices 0 .. ng - 1) column-major, ascending inside a column.  rowptr / cols / vals: V' of all N rows;
 *            max_row = the longest query row.  Each pair is written by exactly one lane and its value does not depend on
 *            which; no floating-point atomics.
 * Every stage returns 0 for N == 0 and checks its limits before anything is launched. */
int creid_rerank_recip(const int64_t* nb, int64_t N, int32_t K, int32_t kh, const int64_t* rowptr, int32_t* count,
                       int32_t* cols, void* stream);
int creid_rerank_weights(const float* X, const float* qq, const float* rowmax, int64_t N, int64_t D,
                         const int64_t* rowptr, const int32_t* cols, float* vals, void* stream);
int creid_rerank_expand(const int64_t* nb, int64_t N, int32_t K, int32_t k2, const int64_t* rowptr, const int32_t* cols,
                        const float* vals, int32_t cap, const int64_t* rowptr2, int32_t* count2, int32_t* cols2,
                        float* vals2, void* stream);
int creid_rerank_blend(const float* dist, const float* rowmax, int64_t nq, int64_t ng, float lambda,
                       const int64_t* rowptr, const int32_t* cols, const float* vals, const int64_t* colptr,
                       const int32_t* colrows, int32_t max_row, float* out, void* stream);

/* ---- neighbour expansion (query expansion / database-side augmentation; csrc/neighbour_expand.hip): the weighted sum of the
 * rows a neighbour table names.  x fp32 [n_src][D]; idx int64 [m][k] with every entry in [0, n_src) (the caller's duty: the
 * kernel does not check it); dist fp32 [m][k], the squared L2 of unit rows as creid_stream_topk_* returns it.
 *   sim = min(max(fmaf(-0.5, dist, 1), 0), 1);  w = 1 when alpha == 0 (dist is then never read and may be NULL), sim when
 *   alpha == 1, else (float)pow((double)sim, (double)alpha);
 *   out[i][c] = sum_t w[i][t] x[idx[i][t]][c]: an fp32 fmaf chain from 0 in the order of t, so a row's bits depend neither on
 *   the launch geometry nor on the other rows of the call.  self_rows fp32 [m][D] (or NULL): row i is the chain's first
 *   addend, at weight 1, before t = 0.
 * out fp32 [m][D] must not overlap x or self_rows.  m == 0 returns 0; CREID_E_ARG for a null pointer, k < 0, n_src < 1 with
 * k > 0, or an alpha that is negative or not finite; CREID_E_SHAPE for D < 4 or D % 4 != 0 (16-byte column chunks) -- all
 * before anything is launched. */
int creid_neighbour_expand(const float* x, int64_t n_src, const int64_t* idx, const float* dist, const float* self_rows,
                           int64_t m, int32_t k, int64_t D, float alpha, float* out, void* stream);

/* Measured launch plans (optional).  kind 0 = weight gradient: key (M = batch*out_h*out_w, out_c, K = kh*kw*in_c, 0) ->
 * (tile rows 64|128, tile cols 64|128, pixel splits | ring depth << 16 | producer/consumer waves << 20 | two k-groups << 21);
 * kind 1 = implicit-GEMM forward / data gradient: key (GEMM rows M, GEMM cols N, K, transposed 0|1 | stride << 1) ->
 * (N tile 64|128, LDS ring depth 2|3|4, kernel 0 producer/consumer | 1 four-wave DMA | 2 persistent 1x1 | 3 256-row tiles |
 * 4 persistent 1x1, second form: forward only, K = 64|128|256, the ring-depth slot caps its column slab: 2 widest, 3 128, 4 64 |
 * 5 all-waves-multiply persistent kernel (conv_pipe.hip): forward only, K % 64 = 0, the first slot is then the variant word
 * tile rows/128 | (tile cols/128) << 2 | k-tiles per phase << 4 | loop form << 8 (0 ping-pong wave groups, 2 free-running),
 * second slot 0).  Key bit 3 of the last component (| 8) marks a plan that applies to the eval-mode epilogue only (folded affine /
 * residual / ReLU): such launches look it up first and fall back to the key without the bit.  A plan only selects among kernel variants
 * the library already has; shapes without an entry use the built-in rules.  Not thread-safe against running launches:
 * register before the first convolution (the Python binding does it at load time from tuned_plans.json). */
int creid_tune_set(int32_t kind, int64_t a, int64_t b, int64_t c, int64_t d, int32_t p0, int32_t p1, int32_t p2);
int creid_tune_clear(void);
/* Host-side use counters of one registered plan: what = 0 -> lookups that returned it, what = 1 -> launches that found it but
 * ran another kernel (a plan word the launch's validity checks reject, a planned kernel that refused the shape, a kernel that
 * takes the shape ahead of every plan).  -1 when (kind, a, b, c, d) is not registered, -2 when `what` is neither 0 nor 1;
 * creid_tune_clear drops the counts with the entries. */
int64_t creid_tune_count(int32_t kind, int64_t a, int64_t b, int64_t c, int64_t d, int32_t what);

/* ------------------------------------------------------------------ stage B: centroids */

/* train_ctl_model.py:79-104: leave-one-out per-PID centroids of a PID-contiguous [P,K] batch.
 * centroids[i,p,:] = sum_{s != i, is_real[p,s]} feat[p*K+s,:] / max(cnt,1) if is_real[p,i] else 0;
 * valid[i,p] = cnt.  feat fp32 [P*K, D]; is_real uint8 [P*K]; centroids fp32 [K,P,D]; valid int32 [K,P]. */
int creid_loo_centroids_fwd(const float* feat, const uint8_t* is_real, int64_t P, int64_t K, int64_t D,
                            float* centroids, int32_t* valid, void* stream);
/* adjoint of the above: dfeat_accum[P*K, D] += J^T dcentroids. */
int creid_loo_centroids_bwd(const float* dcentroids, const uint8_t* is_real, int64_t P, int64_t K,
                            int64_t D, float* dfeat_accum, void* stream);
/* The centroid rounds' operands and scalars without framework glue (train_ctl_model.py:79-124, 143-177):
 * creid_loo_emb_fwd = creid_loo_centroids_fwd that ALSO lays out the K stacked triplet problems: emb [K][2P][D] (round i:
 * the P i-th instances, then the P leave-one-out centroids), lab int64 [K][2P]; creid_loo_emb_bwd adds demb's query rows and
 * the leave-one-out backward of its centroid rows into dfeat [P*K][D]; cnorm [K][P] = L2 norm of every centroid row;
 * creid_ctl_step_stats: out[0..n) = scal * weights, out[n..n+7) = {sum, sum of the K round losses (slots 4, 8, ..), mean over
 * the K rows of scal[4..4K+4) (4 values), mean of the `rows` entries of cnorm}. */
int creid_loo_emb_fwd(const float* feat, const uint8_t* is_real, const int64_t* labels, int64_t P, int64_t K, int64_t D,
                      float* centroids, int32_t* valid, float* emb, int64_t* lab, float* cnorm, void* stream);
int creid_loo_emb_bwd(const float* demb, const uint8_t* is_real, int64_t P, int64_t K, int64_t D, float* dfeat_accum,
                      void* stream);
int creid_ctl_step_stats(const float* scal, const float* weights, int64_t n, int64_t K, const float* cnorm,
                         int64_t rows, float* out, void* stream);

/* ---- the whole head section of a training step in SIX launches (train_ctl_model.py:59-152: everything between the backbone
 * forward and its backward).  The kernels above are latency-bound on a 64 x 2048 feature matrix and four of their chains are
 * independent (query triplet / center loss / BNNeck -> classifier -> cross entropy / centroid rounds): each launch here runs one
 * step of every chain side by side (workgroup roles), in the accumulation order of the sequential calls -- results are
 * bit-identical to them (tests/test_heads_fused_gpu.py).  The last launch also performs creid_gap_bwd of the finished feature
 * gradient, i.e. it hands the backbone its incoming gradient directly.
 *   masked = 0: every row is real (is_real must still be given: all ones); masked = 1: the device-mask schedule below
 *   (creid_*_masked / *_rows semantics, `lonely` required).
 *   loss_weights [4(K+1)+2] / stats [4(K+1)+2+7]: as creid_ctl_step_stats(_rows).  w_centroid: the centroid-triplet weight
 *   (divided by K inside for masked = 0, by the number of valid rounds on the device for masked = 1).
 *   split_logits / split_dbnf: K-splits of the classifier forward / data-gradient GEMMs (1 = single pass, run-to-run identical;
 *   > 1: partial products combined by fp32 atomics like creid_gemm_f32).
 *   d_* are ACCUMULATED into (NULL = not wanted, except d_bn_weight); bn_batches_tracked (nullable) is incremented by one;
 *   amp_state (nullable): f16 loss scale {scale, 1/scale} -- g is multiplied by scale; dfeat_out (nullable, fp32 [B, D]) receives
 *   the unscaled feature gradient; g: [B * HW, D] in g_dtype.  workspace: creid_ctl_heads_workspace_bytes(), 256-byte aligned.
 *   Limits: K <= 16, B <= 256, D % 8 == 0 (else CREID_E_SHAPE: use the separate calls). */
typedef struct creid_ctl_heads {
  int64_t B, P, K, D, num_classes, num_centers, HW;
  int32_t g_dtype, masked, split_logits, split_dbnf;
  float margin, xent_eps, w_query, w_center, w_xent, w_centroid, bn_momentum, bn_eps;
  const float* feat;
  const int64_t* labels;
  const uint8_t* is_real;
  const float* centers;
  const float* bn_weight;
  const float* bn_bias;
  float* bn_running_mean;
  float* bn_running_var;
  const float* fc_weight;
  const float* loss_weights;
  const float* amp_state;
  float* d_centers;
  float* d_bn_weight;
  float* d_bn_bias;
  float* d_fc_weight;
  int64_t* bn_batches_tracked;
  int32_t* lonely;
  float* stats;
  void* g;
  float* dfeat_out;
  void* workspace;
  size_t workspace_bytes;
  /* optional (all five or none; 16-bit g_dtype, D % 256 == 0): the column sums of the BatchNorm backward that consumes g first
   * (the last bottleneck's bn3, modelling/backbones/resnet.py:81-83) are produced by the launch that writes g --
   * bn_partial [creid_bn2d_bwd_rows(B * HW)][2][D], bit-identical to creid_bn2d_bwd's own column pass (partial_ready = 1):
   * bn_x = that layer's raw convolution output [B * HW, D], bn_mask = the ReLU bits of its output, bn_mean / bn_invstd [D]. */
  const void* bn_x;
  const uint8_t* bn_mask;
  const float* bn_mean;
  const float* bn_invstd;
  float* bn_partial;
} creid_ctl_heads;
size_t creid_ctl_heads_workspace_bytes(int64_t B, int64_t P, int64_t K, int64_t D, int64_t num_classes);
int creid_ctl_heads_fused(const creid_ctl_heads* a, void* stream);

/* ---- the same training step for batches with padded samples (isReal = False, datasets/bases.py:346-406), driven by a DEVICE
 * mask so that the step stays free of host synchronisation (hipGraph-capturable for any pattern of fakes):
 *  creid_loo_emb_fwd_rows    = creid_loo_emb_fwd + row_exists uint8 [K][2P]: identity p takes part in round i iff its i-th
 *                              instance is real and it has another real instance (train_ctl_model.py:112-122 keeps these rows);
 *  creid_triplet_fwd_batched_rows: rows with row_exists = 0 are neither anchors nor candidates; a problem with fewer than
 *                              min_rows rows is skipped (out4 = 0, coef = 0: the round with <= 1 valid identity, :113);
 *  creid_ctl_round_scale     : inv_rounds[0] = 1 / #rounds with out4[k][3] >= 4 (the mean over valid rounds, :143-146), the
 *                              gscale_dev of the rounds' creid_triplet_bwd_batched;
 *  creid_ctl_step_stats_rows : creid_ctl_step_stats with the round terms / means over the VALID rounds only and the centroid
 *                              norm averaged per round over its kept rows; weights[4k] must hold the full centroid weight;
 *  *_masked                  : center loss, label-smoothed cross entropy and the BNNeck over the rows with row_mask != 0 only
 *                              (means / statistics over their count), zero gradient and zero output on the others
 *                              (train_ctl_model.py:69-77 feeds features[isReal] to these three). */
int creid_loo_emb_fwd_rows(const float* feat, const uint8_t* is_real, const int64_t* labels, int64_t P, int64_t K, int64_t D,
                           float* centroids, int32_t* valid, float* emb, int64_t* lab, float* cnorm, uint8_t* row_exists,
                           void* stream);
/* creid_loo_emb_fwd_rows that also COUNTS the real instances without a real partner (an identity with exactly one real
 * instance: the reference raises there, train_ctl_model.py:80-104 -> losses/triplet_loss.py:88) into lonely_accum[0] (int32,
 * accumulated with an atomic: the caller zeroes it once per epoch and reads it at the epoch end -- no sync inside the step). */
int creid_loo_emb_fwd_rows_lonely(const float* feat, const uint8_t* is_real, const int64_t* labels, int64_t P, int64_t K, int64_t D,
                                  float* centroids, int32_t* valid, float* emb, int64_t* lab, float* cnorm, uint8_t* row_exists,
                                  int32_t* lonely_accum, void* stream);
int creid_triplet_fwd_batched_rows(const float* x, const int64_t* labels, const uint8_t* row_exists, int64_t nb, int64_t N,
                                   int64_t D, float margin, int32_t min_rows, float* dist_ap, float* dist_an,
                                   int32_t* p_idx, int32_t* n_idx, float* coef, float* out4, void* stream);
int creid_ctl_round_scale(const float* out4_rounds, int64_t K, float* inv_rounds, void* stream);
int creid_ctl_step_stats_rows(const float* scal, const float* weights, int64_t n, int64_t K, int64_t P, const float* cnorm,
                              const uint8_t* row_exists, float* out, void* stream);
int creid_center_loss_fwd_masked(const float* x, const int64_t* labels, const float* centers, const uint8_t* row_mask,
                                 int64_t B, int64_t C, int64_t D, float* row_sq, float* loss, void* stream);
int creid_center_loss_bwd_masked(const float* x, const int64_t* labels, const float* centers, const float* row_sq,
                                 const uint8_t* row_mask, int64_t B, int64_t D, const float* gscale_dev, float gscale,
                                 float* dx_accum, float* dcenters_accum, void* stream);
int creid_xent_ls_masked(const float* logits, const int64_t* targets, const uint8_t* row_mask, int64_t B, int64_t C,
                         float eps, float gscale, float* row_loss, float* loss, float* dlogits, void* stream);
int creid_bn1d_fwd_masked(const float* x, const uint8_t* row_mask, int64_t B, int64_t D, const float* weight,
                          const float* bias, float* running_mean, float* running_var, float momentum, float eps, float* y,
                          float* save_mean, float* save_invstd, void* stream);
int creid_bn1d_bwd_masked(const float* x, const float* dy, const uint8_t* row_mask, int64_t B, int64_t D,
                          const float* weight, const float* save_mean, const float* save_invstd, float* dx_accum,
                          float* dweight_accum, float* dbias_accum, void* stream);

/* ------------------------------------------------------------------ stage C: losses */

/* losses/triplet_loss.py:27-41 (euclidean_dist), :68-119 (hard_example_mining), :139-173
 * (TripletLoss.__call__).  x fp32 [N,D]; labels int64 [N]; anchor_mask uint8 [N] or NULL (applied
 * AFTER mining, :148-151).  margin >= 0 -> MarginRankingLoss(margin); margin < 0 -> SoftMarginLoss.
 * Outputs: dist_ap/dist_an fp32 [N] (all anchors, unmasked), p_idx/n_idx int32 [N] (first index wins
 * ties), coef fp32 [N] (= dloss/d dist_ap, nullable), out4 = {loss, mean ap, mean an, #anchors} over
 * masked anchors, dist_mat fp32 [N,N] (nullable; the sqrt(clamp(.,1e-12)) matrix). */
int creid_triplet_fwd(const float* x, const int64_t* labels, const uint8_t* anchor_mask, int64_t N,
                      int64_t D, float margin, float* dist_ap, float* dist_an, int32_t* p_idx,
                      int32_t* n_idx, float* coef, float* out4, float* dist_mat, void* stream);
/* dx_accum[N,D] += gscale * (*gscale_dev if non-NULL) * dloss/dx (zero through an active clamp). */
int creid_triplet_bwd(const float* x, int64_t N, int64_t D, const float* dist_ap, const float* dist_an,
                      const int32_t* p_idx, const int32_t* n_idx, const float* coef,
                      const float* gscale_dev, float gscale, float* dx_accum, void* stream);

/* nb independent problems of the same size in one launch each (the K centroid rounds of
 * train_ctl_model.py:112-148): every array of creid_triplet_fwd / _bwd gains a leading [nb] dimension
 * (x [nb][N][D], labels / dist_* / *_idx / coef / anchor_mask [nb][N], out4 [nb][4], dx_accum [nb][N][D]). */
int creid_triplet_fwd_batched(const float* x, const int64_t* labels, const uint8_t* anchor_mask, int64_t nb,
                              int64_t N, int64_t D, float margin, float* dist_ap, float* dist_an,
                              int32_t* p_idx, int32_t* n_idx, float* coef, float* out4, float* dist_mat,
                              void* stream);
int creid_triplet_bwd_batched(const float* x, int64_t nb, int64_t N, int64_t D, const float* dist_ap,
                              const float* dist_an, const int32_t* p_idx, const int32_t* n_idx,
                              const float* coef, const float* gscale_dev, float gscale, float* dx_accum,
                              void* stream);

/* SOLVER.DISTANCE_FUNC = 'cosine' (losses/triplet_loss.py:44-65,134-137): the same mining / loss / backward on
 * the cosine distance clamp(|1 - x_i.x_j|, 1e-12) of rows already scaled to unit length (x_unit =
 * creid_rownorm_fwd(mode 0) of the features).  Argument meaning as creid_triplet_fwd / _bwd; the backward is
 * with respect to x_unit (chain creid_rownorm_bwd for the raw features). */
int creid_triplet_cosine_fwd(const float* x_unit, const int64_t* labels, const uint8_t* anchor_mask, int64_t N,
                             int64_t D, float margin, float* dist_ap, float* dist_an, int32_t* p_idx,
                             int32_t* n_idx, float* coef, float* out4, float* dist_mat, void* stream);
int creid_triplet_cosine_bwd(const float* x_unit, int64_t N, int64_t D, const float* dist_ap,
                             const float* dist_an, const int32_t* p_idx, const int32_t* n_idx,
                             const float* coef, const float* gscale_dev, float gscale, float* dx_accum,
                             void* stream);

/* Row scaling to unit length: mode 0  y = x / max(|x|_2, eps)  (cosine_similarity, losses/triplet_loss.py:50-52);
 * mode 1  y = x / (|x|_2 + eps)  (`normalize`, losses/triplet_loss.py:16-24, used by normalize_feature=True).
 * norm[N] receives |x|_2 (saved for the backward).  bwd: dx = d(y)/d(x)^T dy (overwrites dx). */
int creid_rownorm_fwd(const float* x, int64_t N, int64_t D, int mode, float eps, float* y, float* norm,
                      void* stream);
int creid_rownorm_bwd(const float* x, const float* norm, const float* dy, int64_t N, int64_t D, int mode,
                      float eps, float* dx, void* stream);

/* hard_example_mining(dist_mat, labels, return_inds=True) of losses/triplet_loss.py:68-119 on a GIVEN
 * square distance matrix fp32 [N,N]: hardest positive (max, self included) / hardest negative (min) per
 * anchor row, first index wins ties. */
int creid_hard_mine_from_dist(const float* dist_mat, const int64_t* labels, int64_t N, float* dist_ap,
                              float* dist_an, int32_t* p_idx, int32_t* n_idx, void* stream);

/* d[i] = sqrt(max(d[i], lo)) in place: the `clamp(min=1e-12).sqrt()` tail of euclidean_dist(x, y)
 * (losses/triplet_loss.py:40) after creid_sqdist_matrix. */
int creid_clamp_sqrt_inplace(float* d, int64_t n, float lo, void* stream);

/* losses/center_loss.py:26-46.  row_sq[b] = |x_b|^2 + |c_y|^2 - 2 x_b.c_y (unclamped, saved for bwd);
 * loss[0] = (sum_b clamp(row_sq[b],1e-12,1e12) + B*(C-1)*1e-12) / B. */
int creid_center_loss_fwd(const float* x, const int64_t* labels, const float* centers, int64_t B,
                          int64_t C, int64_t D, float* row_sq, float* loss, void* stream);
/* dx_accum[B,D] += g*(2/B)(x_b - c_y); dcenters_accum[C,D] += g*(2/B) sum_{b:y_b=y}(c_y - x_b) on the
 * touched rows only (either output may be NULL). */
int creid_center_loss_bwd(const float* x, const int64_t* labels, const float* centers,
                          const float* row_sq, int64_t B, int64_t D, const float* gscale_dev,
                          float gscale, float* dx_accum, float* dcenters_accum, void* stream);

/* losses/triplet_loss.py:194-205 CrossEntropyLabelSmooth: loss[0] = mean_b(-sum_c t_c logp_c),
 * t = (1-eps)*onehot + eps/C; dlogits (nullable) = gscale * (softmax - t) / B. */
int creid_xent_ls(const float* logits, const int64_t* targets, int64_t B, int64_t C, float eps,
                  float gscale, float* row_loss, float* loss, float* dlogits, void* stream);

/* modelling/bases.py:83-84 BNNeck = nn.BatchNorm1d(D) on [B,D] (momentum 0.1, eps 1e-5):
 * training: batch stats (biased var for y, unbiased into running_var); eval: running stats. */
int creid_bn1d_fwd(const float* x, int64_t B, int64_t D, const float* weight, const float* bias,
                   float* running_mean, float* running_var, int training, float momentum, float eps,
                   float* y, float* save_mean, float* save_invstd, void* stream);
int creid_bn1d_bwd(const float* x, const float* dy, int64_t B, int64_t D, const float* weight,
                   const float* save_mean, const float* save_invstd, float* dx_accum,
                   float* dweight_accum, float* dbias_accum, void* stream);

/* modelling/bases.py:92-95,238-241 (validation_create_centroids): out[s,:] = mean of the rows
 * emb[order[j],:], j in [offsets[s], offsets[s+1]) (summed in list order). */
int creid_gather_mean_rows(const float* emb, const int64_t* order, const int64_t* offsets,
                           int64_t n_seg, int64_t D, float* out, void* stream);

/* ------------------------------------------------------------------ optimiser steps */

/* solver/build.py:36-39 torch.optim.Adam (L2 weight decay added to the gradient, bias correction,
 * eps outside the sqrt) over a flat fp32 buffer; the gradient is multiplied by grad_scale first. */
int creid_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                    float beta2, float eps, float weight_decay, int64_t step, float grad_scale,
                    void* stream);
/* Same update with the step-dependent scalars resident on the device: hyper_dev = float[8]
 * {lr, step, 1-beta1^step, sqrt(1-beta2^step), ticket (int32, must be 0 between calls), 3 reserved}; the
 * call uses step + 1 and its bias corrections and leaves them in hyper_dev (written by the last
 * workgroup of the one launch), so a captured hipGraph replays correctly; the host only rewrites
 * hyper_dev[0] when the learning rate changes.  n % 4 == 0. */
int creid_adam_step_dev(float* p, const float* g, float* m, float* v, int64_t n, float* hyper_dev,
                        float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                        void* stream);
/* train_ctl_model.py:157-159 + solver/build.py:44: g *= grad_mul (in place); p -= lr * g. */
int creid_sgd_scaled_step(float* p, float* g, int64_t n, float lr, float grad_mul, void* stream);

/* f16 mixed-precision training -- the reference's own mixed precision (utils/misc.py:111 `precision=16`, i.e. native AMP with
 * torch.cuda.amp.GradScaler under pytorch-lightning 1.1.4) -- with the dynamic loss scale RESIDENT ON THE DEVICE, so that the
 * step contains no host synchronisation and a captured hipGraph replays through overflow steps:
 *   amp_state = float[2] {scale, 1 / scale}; amp_flags = int32[3] {found_inf of this step, clean steps in a row, steps
 *   skipped in total}.
 * creid_amp_scale          y = x * scale (the head gradient entering the f16 backbone backward);
 * creid_amp_unscale_check  g *= 1 / scale in place over n (% 4 == 0) floats, any non-finite element sets amp_flags[0];
 * creid_adam_step_dev_amp / creid_sgd_scaled_step_amp  = the plain steps, skipped entirely (Adam's step counter included) while
 *                          *skip_flag != 0 (GradScaler.step);
 * creid_amp_update         found_inf ? scale *= backoff : (after growth_interval clean steps) scale *= growth; clears found_inf
 *                          (GradScaler.update; scale clamped to [1, 2^24]). */
int creid_amp_scale(const float* x, int64_t n, const float* amp_state, float* y, void* stream);
int creid_amp_unscale_check(float* g, int64_t n, const float* amp_state, int32_t* amp_flags, void* stream);
int creid_amp_update(float* amp_state, int32_t* amp_flags, float growth_factor, float backoff_factor, int32_t growth_interval,
                     void* stream);
int creid_adam_step_dev_amp(float* p, const float* g, float* m, float* v, int64_t n, float* hyper_dev, float beta1, float beta2,
                            float eps, float weight_decay, float grad_scale, const int32_t* skip_flag, void* stream);
int creid_sgd_scaled_step_amp(float* p, float* g, int64_t n, float lr, float grad_mul, const int32_t* skip_flag, void* stream);

/* ------------------------------------------------------------------ small fp32 GEMM */

/* Classifier of the BNNeck head (modelling/bases.py:86-87 fc_query = Linear(D -> C, bias=False);
 * used at train_ctl_model.py:75): C[m,n] = alpha * sum_k A[m*sam + k*sak] * B[k*sbk + n*sbn]
 * + beta * C[m*ldc + n], exact-f32 MFMA.  split_k > 1 combines K-slices with fp32 atomics
 * (non-deterministic order); split_k == 1 is deterministic. */
int creid_gemm_f32(const float* A, int64_t sam, int64_t sak, const float* B, int64_t sbk, int64_t sbn,
                   float* C, int64_t ldc, int64_t M, int64_t N, int64_t K, float alpha, float beta,
                   int32_t split_k, void* stream);

/* ------------------------------------------------------------------ stage A: backbone layers */

/* Convolution geometry (NHWC activations; square kernels 1x1 / 3x3, stride 1 or 2; channel counts
 * powers of two >= 64 -- every non-stem convolution of modelling/backbones/resnet.py:51-120). */
typedef struct {
  int64_t batch, in_h, in_w, in_c, out_h, out_w, out_c;
  int32_t kh, kw, stride, pad;
} creid_conv_desc;

/* nn.Conv2d forward (resnet.py:56-61,109): y[b,oy,ox,n] = sum_{r,s,c} x[b,oy*st+r-pad,ox*st+s-pad,c] *
 * w_krsc[n,r,s,c]; im2col-free implicit GEMM on the MFMA pipe (bf16 -> fp32 accumulate, or exact f32).
 * bn_partial (nullable) receives per-128-row-tile (sum, sumsq) of the fp32 accumulators,
 * float [creid_conv2d_bn_partial_rows(d)][2][out_c], for the BatchNorm that follows. */
int64_t creid_conv2d_bn_partial_rows(const creid_conv_desc* d);
/* Launches so far (this process) of the resident-halo form of the producer/consumer kernel: stride-1 3x3 forward / data
 * gradient, 64 | 128 | 256 channels, 128-row tiles of whole image rows; CREID_IGEMM_HALO=0 turns it off.  Same bits either way. */
int64_t creid_igemm_halo_launches(void);
/* Launches so far (this process) of the tap-fused weight-gradient kernel (wgrad_bf16_taps_kernel): 16-bit stride-1 pad-1 3x3
 * layers with in_c in {64, 128, 256, 512}, out_c % 64 == 0, out_w in {8, 16, 32} and out_h * out_w % 128 == 0 -- one workgroup
 * per (64 co x 64 ci x nine taps) over its pixel range.  CREID_WGRAD_TAPS=0 (read per call) restores the per-tap tile launches
 * with their split counts and workspace sizes. */
int64_t creid_wgrad_taps_launches(void);
/* Which kernel a convolution call would run, as one line of text -- decided by the same code the launchers run, without
 * launching: host only, no device API, the plan registry is peeked at (creid_tune_count does not move), so it answers in a
 * process that has no GPU (the CU count behind the persistent grids then falls back to the MI355X's 256).
 *   op: CREID_ROUTE_FWD / DGRAD / WGRAD take d; CREID_ROUTE_STEM_FWD / STEM_WGRAD read (batch, in_h, in_w) = (B, H, W) of d.
 *   feat_bits: the facts of the call that steer routing, CREID_ROUTE_* below.  CREID_ROUTE_JOB: a carried job comes with the
 *     call, of (feat_bits >> 16) workgroups -- the previous weight gradient's split reduction for a data gradient, the
 *     BatchNorm-backward finalize job for a weight gradient (its partials launch).
 *   buf[n] receives, NUL-terminated,
 *       [pre=wred(N) ; ]<kernel instantiation> grid=(x,y,1) block=B lds=L[ parity=1][ wred=N][ fin=N][ ; post=fin(N)] | plan=...
 *     or  rc=<CREID_E_*> | plan=...  where no kernel covers the call.  pre / post: a job that cannot ride runs as its own launch
 *     before / after; wred / fin: it rides in the grid.  plan=none | hit | declined (what creid_tune_count would record), then
 *     the key slot, the planned and the running kernel id (forward / data gradient) or the split plan (weight gradient).
 * Returns 0, CREID_E_ARG, or CREID_E_WS when n is too small (the text is then truncated). */
enum { CREID_ROUTE_FWD = 0, CREID_ROUTE_DGRAD = 1, CREID_ROUTE_WGRAD = 2, CREID_ROUTE_STEM_FWD = 3, CREID_ROUTE_STEM_WGRAD = 4 };
enum { CREID_ROUTE_ADD = 1, CREID_ROUTE_ADD_COMPACT = 2, CREID_ROUTE_ADD_MASK = 4, CREID_ROUTE_STATS = 8, CREID_ROUTE_AFFINE = 16,
       CREID_ROUTE_BNRED = 32, CREID_ROUTE_BNRED_PER_IMAGE = 64, CREID_ROUTE_JOB = 128 };
int creid_conv_route_describe(const creid_conv_desc* d, int op, int feat_bits, int dtype, char* buf, size_t n);
int creid_conv2d_fwd_nhwc(const creid_conv_desc* d, const void* x, const void* w_krsc, void* y,
                          float* bn_partial, int dtype, void* stream);
/* Eval-mode forward of conv -> BatchNorm -> (+ residual) -> (ReLU) in ONE launch (modelling/backbones/resnet.py:67-87 under
 * model.eval(), the path of validation_step, modelling/bases.py:169-177, and of inference/inference_utils.py:104-113): with
 * running statistics BatchNorm is the per-channel affine scale_shift = float[2][out_c] {gamma / sqrt(var + eps),
 * beta - mean * scale} (creid_bn2d_fold_multi), applied to the fp32 accumulators in the epilogue:
 * y = act(conv(x) * scale + shift (+ residual)), act = ReLU when relu != 0; residual (nullable) has y's shape and dtype.
 * Same arithmetic as creid_conv2d_fwd_nhwc + creid_bn2d_finalize(training = 0) + creid_bn2d_apply, without the two extra
 * passes (fp32 mode: bit-identical; bf16 mode: the conv output is rounded once, after the affine, instead of twice).
 * dtype CREID_BF16X3 (this call and creid_conv2d_fwd_nhwc, bn_partial included): x, y and residual fp32, w_krsc the two-plane
 * bf16 buffer [2][out_c][kh][kw][in_c] of creid_weight_prep; the k order of every output element is fixed by the shape alone
 * (identical bits whatever the batch size). */
int creid_conv2d_fwd_affine_nhwc(const creid_conv_desc* d, const void* x, const void* w_krsc, void* y,
                                 const float* scale_shift, const void* residual, int relu, int dtype, void* stream);
/* Training forward of a 1 x 1 stride-1 convolution whose INPUT is still the raw output of the previous convolution: that layer's
 * training-mode BatchNorm + ReLU (scale_shift [2][K] from creid_bn2d_finalize: a = max(x * scale + shift, 0), the arithmetic of
 * creid_bn2d_apply_mask) is applied on the operand path -- conv3 of a Bottleneck consuming conv2's raw output
 * (modelling/backbones/resnet.py:73-78) without the stand-alone apply pass.  y [M, N] (+ bn_partial like creid_conv2d_fwd_nhwc);
 * a_out [M, K] and mask_out [M * K / 8] (both or neither): the normalised tensor and its ReLU bits, bit-identical to
 * creid_bn2d_apply_mask's (the backward reads them).  16-bit dtypes, K in {64, 128}, N % 64 == 0; else CREID_E_SHAPE. */
int creid_conv1x1_bnrelu_fwd(const void* x_raw, const float* scale_shift, const void* w_krsc, int64_t M, int64_t K, int64_t N,
                             void* y, float* bn_partial, void* a_out, uint8_t* mask_out, int dtype, void* stream);
/* Folds MANY BatchNorm layers in one launch.  table_dev = device array of n_entries records { const float* gamma (nullable);
 * const float* beta (nullable); const float* running_mean; const float* running_var; float* out (float[2][C]); int32 C;
 * float eps } (48 bytes, creid_bn2d_fold_entry_bytes()). */
int64_t creid_bn2d_fold_entry_bytes(void);
int creid_bn2d_fold_multi(const void* table_dev, int64_t n_entries, void* stream);
/* data gradient: dx = conv_transpose(dy, w) (+ add_src if non-NULL); w_crsk is [in_c][kh][kw][out_c]. */
int creid_conv2d_dgrad_nhwc(const creid_conv_desc* d, const void* dy, const void* w_crsk, void* dx,
                            const void* add_src, int dtype, void* stream);
/* bf16x3 data gradient (CREID_BF16X3 arithmetic, three bf16 MFMAs per product): dx = conv_transpose(dy, w) (+ add_src if
 * non-NULL).  dy, dx and add_src fp32 NHWC ([batch, out_h, out_w, out_c] in, [batch, in_h, in_w, in_c] out and add_src);
 * w2_crsk = bf16 [2][in_c][kh][kw][out_c], hi plane then lo plane (creid_weight_prep_x3_train_multi).  The k order of every
 * element is fixed by the shape (every tap of the kernel, absent taps of a stride-2 layer contributing zeros).
 * Returns CREID_E_ARG for a null pointer, CREID_E_SHAPE for a descriptor outside the convolution kernels' cover (in_c and
 * out_c powers of two >= 64, 1 x 1 or 3 x 3, stride 1 or 2), before anything is launched. */
int creid_conv2d_dgrad_x3_nhwc(const creid_conv_desc* d, const void* dy, const void* w2_crsk, void* dx, const void* add_src,
                               void* stream);
/* The same data gradient with the column reduction of the NEXT BatchNorm backward fused into the epilogue
 * (bf16 only): dx is g = dL/da of the layer whose raw conv output is bn_x and post-ReLU activation bn_act
 * (nullable); bn_partial[ceil(M/128)][2][in_c] receives (sum dy, sum dy*xhat), dy = g*[bn_act > 0].
 * bn_stat_image_rows = 0: bn_mean/bn_invstd are float[in_c] (BatchNorm); = in_h*in_w (a multiple of 128): they
 * are float[batch][in_c], per-(image, channel) statistics of an IBN layer (creid_ibn_bwd, partial_ready).
 * add_src_stride = 1: add_src is [batch, in_h, in_w, in_c]; = 2: add_src is the COMPACT gradient of a stride-2
 * 1x1 downsample branch, [batch, in_h/2, in_w/2, in_c], added at even (y, x) only (Bottleneck with stride,
 * resnet.py:87-88: its full-resolution data gradient is never materialised). */
int creid_conv2d_dgrad_bnred_nhwc(const creid_conv_desc* d, const void* dy, const void* w_crsk, void* dx,
                                  const void* add_src, const void* bn_x, const void* bn_act,
                                  const float* bn_mean, const float* bn_invstd, float* bn_partial,
                                  int64_t bn_stat_image_rows, int add_src_stride, int dtype, void* stream);

/* The data gradient with everything that can ride in the same launch: "+ add_src" (add_src_stride as above; the compact
 * form exists in the 16-bit LDS-DMA kernels and in the fp32 kernel), the
 * NEXT BatchNorm-backward's column reduction (bn_x != NULL, arguments as creid_conv2d_dgrad_bnred_nhwc), and the
 * split reduction of the PREVIOUS weight-gradient launch: wred_desc != NULL names the convolution whose
 * creid_conv2d_wgrad_partials call filled wred_ws; the first workgroups of this launch sum those partials into
 * wred_dw (OIHW fp32; wred_accumulate as in creid_conv2d_wgrad_nhwc) while the rest compute gradient tiles, so the
 * 5-25 us stand-alone reduce launch per layer disappears.  In fp32 parity mode the reduction runs as its own launch
 * first (same result).  bn_mask != NULL: the ReLU mask of that BatchNorm's output as bits (creid_bn2d_apply_mask) --
 * one byte per 8 channels is read instead of the 16 bytes of bn_act.  add_mask != NULL (add_src_stride 1, bf16): add_src
 * is multiplied by those ReLU bits before the add -- the residual branch then takes the block's UNMASKED incoming
 * gradient, and the masked copy creid_bn2d_bwd would write through gm_out is never materialised. */
int creid_conv2d_dgrad_fused_nhwc(const creid_conv_desc* d, const void* dy, const void* w_crsk, void* dx,
                                  const void* add_src, int add_src_stride, const uint8_t* add_mask, const void* bn_x,
                                  const void* bn_act, const uint8_t* bn_mask, const float* bn_mean, const float* bn_invstd,
                                  float* bn_partial, int64_t bn_stat_image_rows, const creid_conv_desc* wred_desc, float* wred_dw,
                                  int wred_accumulate, const void* wred_ws, size_t wred_ws_bytes, int dtype,
                                  void* stream);
/* weight gradient into the fp32 OIHW tensor (the reference's nn.Parameter layout), optionally
 * accumulating; the pixel reduction is split over workgroups through `ws`. */
size_t creid_conv2d_wgrad_workspace_bytes(const creid_conv_desc* d, int dtype);
int creid_conv2d_wgrad_nhwc(const creid_conv_desc* d, const void* x, const void* dy, float* dw_oihw,
                            int accumulate, void* ws, size_t ws_bytes, int dtype, void* stream);
/* The two halves of the call above as separate launches (same workspace contents in between): the split
 * reduce is a short, memory-light kernel that a caller may put on a second stream beside the next data gradient. */
int creid_conv2d_wgrad_partials(const creid_conv_desc* d, const void* x, const void* dy, void* ws,
                                size_t ws_bytes, int dtype, void* stream);
/* A BatchNorm-backward finalize (arguments as in creid_conv2d_wgrad_partials_bnfin) and the split reduction of a weight
 * gradient (arguments as in creid_conv2d_wgrad_reduce_job) in ONE launch: independent pieces of work, one latency-bound and
 * one bandwidth-bound.  Afterwards creid_bn2d_bwd_mask(..., partial_ready = 2, ...). */
int creid_bn2d_bwd_finalize_wred(const float* bn_partial, int64_t bn_rows, int64_t bn_C, int64_t bn_count,
                                 const float* bn_mean, const float* bn_invstd, const float* bn_gamma, float* bn_sums,
                                 float* bn_dgamma, float* bn_dbeta, const creid_conv_desc* wred_desc, float* wred_dw,
                                 int wred_accumulate, const void* wred_ws, size_t wred_ws_bytes, int dtype, void* stream);
/* creid_conv2d_wgrad_reduce with the summation order of the carried form (the job creid_conv2d_dgrad_fused_nhwc runs in its
 * last workgroups): a reduction that finds no carrier gives bit-identical gradients to one that did. */
int creid_conv2d_wgrad_reduce_job(const creid_conv_desc* d, float* dw_oihw, int accumulate, const void* ws,
                                  size_t ws_bytes, int dtype, void* stream);
/* bf16x3 weight gradient: dW[o][c][r][s] = sum over pixels of dy * x with both fp32 operands split into (hi, lo) bf16 and
 * three bf16 MFMAs per product (fp32 accumulation).  x fp32 [batch, in_h, in_w, in_c], dy fp32 [batch, out_h, out_w, out_c].
 * The partial tiles use exactly the workspace of the fp32 weight gradient: layout [split][out_c][kh*kw*in_c] fp32 with the
 * split count of creid_conv2d_wgrad_workspace_bytes(d, CREID_F32), which is what creid_conv2d_wgrad_x3_workspace_bytes
 * returns (0 for a descriptor outside the cover).  creid_conv2d_wgrad_x3_partials writes the partial tiles only; they are
 * summed with dtype CREID_F32 by creid_conv2d_wgrad_reduce_job (or creid_conv2d_wgrad_reduce, or carried by
 * creid_bn2d_bwd_finalize_wred / creid_conv2d_dgrad_fused_nhwc with CREID_F32), deterministically.
 * creid_conv2d_wgrad_x3_nhwc = partials + creid_conv2d_wgrad_reduce_job(CREID_F32): bit-identical to the two-call form.
 * dw_oihw fp32 OIHW, accumulate as in creid_conv2d_wgrad_nhwc.  Returns CREID_E_ARG for a null pointer, CREID_E_SHAPE for a
 * descriptor outside the cover, CREID_E_WS for a short workspace -- all before anything is launched. */
size_t creid_conv2d_wgrad_x3_workspace_bytes(const creid_conv_desc* d);
int creid_conv2d_wgrad_x3_nhwc(const creid_conv_desc* d, const void* x, const void* dy, float* dw_oihw, int accumulate,
                               void* ws, size_t ws_bytes, void* stream);
int creid_conv2d_wgrad_x3_partials(const creid_conv_desc* d, const void* x, const void* dy, void* ws, size_t ws_bytes,
                                   void* stream);
/* creid_conv2d_wgrad_partials whose launch also carries a BatchNorm-backward FINALIZE in its first workgroups: the weight
 * gradient is independent of the chain dgrad -> finalize -> apply -> dgrad, so issued between a data gradient and the next
 * BatchNorm's apply it hides that 4-128-workgroup, latency-bound step (bn_*: the arguments creid_bn2d_bwd's finalize
 * takes -- partial [bn_rows][2][bn_C] as written by the fused data gradient, count = rows of the statistics).  Afterwards
 * call creid_bn2d_bwd_mask(..., partial_ready = 2, sums = bn_sums, ...): apply only. */
int creid_conv2d_wgrad_partials_bnfin(const creid_conv_desc* d, const void* x, const void* dy, void* ws, size_t ws_bytes,
                                      int dtype, const float* bn_partial, int64_t bn_rows, int64_t bn_C, int64_t bn_count,
                                      const float* bn_mean, const float* bn_invstd, const float* bn_gamma, float* bn_sums,
                                      float* bn_dgamma, float* bn_dbeta, void* stream);
int creid_conv2d_wgrad_reduce(const creid_conv_desc* d, float* dw_oihw, int accumulate, const void* ws,
                              size_t ws_bytes, int dtype, void* stream);

/* Stem (resnet.py:94): Conv2d(3, 64, 7, stride 2, pad 3) on the zero-padded NHWC4 image
 * xpad [B, H+8, W+6, 4] made by creid_image_to_nhwc4_pad; w_stem [64][8][32] from creid_stem_weight_prep.
 * Every stem call below (the three forwards, the weight gradient and its workspace size) refuses, before anything is launched:
 * CREID_E_ARG a null pointer or a non-positive batch, H or W; CREID_E_SHAPE an odd H or W, batch * (H/2) * (W/2) >= 2^24 (the
 * kernels decompose an output row into (image, y, x) with fp32 reciprocals, exact below 2^24 only -- the limit of every other
 * convolution) and batch * (H+8) * (W+6) > 2^31 - 1 (they index the padded image's pixels in 32 bits). */
int creid_stem_conv_fwd(int64_t batch, int64_t H, int64_t W, const void* xpad, const void* w_stem, void* y,
                        float* bn_partial, int dtype, void* stream);
/* the stem with its eval-mode BatchNorm (scale_shift float[2][64]) and optional ReLU (resnet_ibn_a.py:129) folded in */
int creid_stem_conv_fwd_affine(int64_t batch, int64_t H, int64_t W, const void* xpad, const void* w_stem, void* y,
                               const float* scale_shift, int relu, int dtype, void* stream);
/* The whole eval-mode stem in one launch (resnet.py:95-98,123-126: conv1 -> bn1 -> [relu] -> maxpool): creid_stem_conv_fwd_affine +
 * creid_maxpool3x3s2_fwd without the full-resolution tensor in between; y [batch, H/4, W/4, 64], bit-identical to the two calls.
 * 16-bit dtypes; CREID_E_SHAPE for image sizes outside the kernel's tiles (W = 128 or 320 with H % 8 = 0): the
 * caller then makes the two calls. */
int creid_stem_conv_pool_fwd_affine(int64_t batch, int64_t H, int64_t W, const void* xpad, const void* w_stem, void* y,
                                    const float* scale_shift, int relu, int dtype, void* stream);
/* Eval-mode block boundary of layer1 in one launch (resnet.py:77-87 of bottleneck i, then :69-71 of bottleneck i + 1):
 * out3 = relu(conv3(a2) * scale3 + shift3 + residual)   [M, c_out]   (= creid_conv2d_fwd_affine_nhwc with residual and ReLU)
 * out1 = relu(conv1_next(out3) * scale1 + shift1)       [M, c_next]  (= creid_conv2d_fwd_affine_nhwc on out3)
 * both 1 x 1 stride 1; a2 [M, c_mid]; weights in the [O][I] layout of creid_weight_prep; fold3 float[2][c_out], fold1
 * float[2][c_next].  The block output is written once and never read back; both outputs are bit-identical to the two calls.
 * 16-bit dtypes, (c_mid, c_out, c_next) = (64, 256, 64) only -- anything else: CREID_E_SHAPE, the caller makes the two calls. */
int creid_bottleneck_c3_c1_fwd_affine(int64_t M, int64_t c_mid, int64_t c_out, int64_t c_next, const void* a2, const void* w3_krsc,
                                      const float* fold3, const void* residual, void* out3, const void* w1_krsc,
                                      const float* fold1, void* out1, int dtype, void* stream);
/* The same launch when the next block's conv1 feeds an IBN layer (resnet_ibn_a.py:27-32): out1_raw [M, c_next] is the raw
 * convolution output and bn_partial1 float[M / 128][2][c_next] its per-128-row (sum, sum of squares) -- what creid_conv2d_fwd_nhwc
 * hands to creid_ibn_fwd (rows of a tile belong to one image when H * W % 128 = 0); M % 128 = 0 required. */
int creid_bottleneck_c3_c1_fwd_stats(int64_t M, int64_t c_mid, int64_t c_out, int64_t c_next, const void* a2, const void* w3_krsc,
                                     const float* fold3, const void* residual, void* out3, const void* w1_krsc, void* out1_raw,
                                     float* bn_partial1, int dtype, void* stream);
/* Stem weight gradient into the fp32 OIHW [64, 3, 7, 7] tensor (dy [batch, H/2, W/2, 64]; accumulate, ws as in
 * creid_conv2d_wgrad_nhwc).  creid_stem_conv_wgrad_workspace_bytes returns 0 for a shape the stem calls refuse (above):
 * creid_stem_conv_wgrad then returns that refusal whatever workspace it is given. */
size_t creid_stem_conv_wgrad_workspace_bytes(int64_t batch, int64_t H, int64_t W, int dtype);
int creid_stem_conv_wgrad(int64_t batch, int64_t H, int64_t W, const void* xpad, const void* dy,
                          float* dw_oihw, int accumulate, void* ws, size_t ws_bytes, int dtype, void* stream);
int creid_image_to_nhwc4_pad(const float* x_nchw, int64_t B, int64_t H, int64_t W, int dtype, void* xpad,
                             void* stream);
/* Input transforms after the Resize (datasets/transforms/build.py:16-31, datasets/transforms/random_erasing.py:31-55) on a whole
 * uint8 batch: RandomHorizontalFlip -> Pad(pad, 0) -> RandomCrop(H, W) -> ToTensor -> Normalize -> RandomErasing, as a pure
 * function of the pixels and of the host-made draws.  src_hwc: uint8 [B, H, W, 3]; params: int32 [B, 8] =
 * {flip, crop_top, crop_left, erase, x1, y1, h, w} (crop offsets in the (H + 2 pad) x (W + 2 pad) padded frame; the erased block
 * is rows x1..x1+h, columns y1..y1+w of the output and receives (erase0, erase1, erase2) AS IS -- the reference writes
 * PIXEL_MEAN into the normalised tensor); params NULL = the test transform (ToTensor + Normalize only, pad must be 0).
 * layout 0: fp32 NCHW [B, 3, H, W] (dtype must be CREID_F32); layout 1: the stem's operand, zero-padded NHWC4
 * [B, H + 8, W + 6, 4] in `dtype` (f32 | bf16), identical to creid_image_to_nhwc4_pad of the layout-0 result. */
int creid_augment_u8(const uint8_t* src_hwc, const int32_t* params, int64_t B, int64_t H, int64_t W, int64_t pad,
                     float mean0, float mean1, float mean2, float std0, float std1, float std2, float erase0, float erase1,
                     float erase2, int32_t layout, int32_t dtype, void* out, void* stream);
/* The Resize in front of those transforms (datasets/transforms/build.py:17,28: T.Resize((H, W)) on a PIL RGB image =
 * Image.resize((W, H), BILINEAR)) on a ragged uint8 batch, EQUAL to Pillow's result byte for byte.
 *   src: `src_bytes` bytes, the images packed back to back as HWC RGB; offsets: int64 [B], byte offset of each image (any
 *   alignment); sizes: int32 [B, 2] = (h, w), sides 1..16384; out: uint8 [B, H, W, 3], H and W 1..4096 -- the tensor
 *   creid_augment_u8 takes.  tables: `table_len` int32 holding one coefficient table per distinct (source side -> target side)
 *   pair of the batch; table_offsets: int32 [B, 2] = where the image's (w -> W) and (h -> H) tables start.
 * Arithmetic (Pillow's 8-bit resample; per axis with `in` source and `out` target samples, in float64 on the host):
 *   scale = in / out; fs = max(scale, 1); ksize = 2 ceil(fs) + 1; for output sample xx: center = (xx + 0.5) scale,
 *   xmin = max((int)(center - fs + 0.5), 0), xmax = min((int)(center + fs + 0.5), in), n = xmax - xmin; tap x < n weighs
 *   w = max(0, 1 - |(x + xmin - center + 0.5) (1 / fs)|), divided by the sum of the w in tap order; k = (int)(w 2^22 + 0.5).
 *   A table is {xmin, n} for each of the `out` samples, then ksize coefficients for each (k[0..n), zero beyond); in == out is
 *   the identity table (xmin = xx, n = 1, k = 2^22, ksize 3).
 *   On the device, integers only: the horizontal pass first, sample = clip8((2^21 + sum_x k[x] pixel[xmin + x]) >> 22) per
 *   channel in int32, ROUNDED TO uint8, then the vertical pass over those values in the same way.  The intermediate image is
 *   never written to memory.
 * Only the pointers and B, H, W, src_bytes, table_len can be checked on the host (CREID_E_ARG before any launch).  The kernel
 * itself refuses whatever the device-side metadata would send out of bounds: an image whose extent does not fit `src_bytes`,
 * whose sides are outside 1..16384 or whose tables do not fit `table_len` comes out black, and tap ranges are clamped into
 * the image. */
int creid_resize_u8(const uint8_t* src, int64_t src_bytes, const int64_t* offsets, const int32_t* sizes, const int32_t* tables,
                    int64_t table_len, const int32_t* table_offsets, int64_t B, int64_t H, int64_t W, uint8_t* out,
                    void* stream);
/* fp32 OIHW master weights -> compute-dtype [O][r][s][I] (forward) and [I][r][s][O] (dgrad, nullable).
 * CREID_BF16X3: w_krsc = bf16 [2][O][r][s][I], hi plane then lo plane; w_crsk must be NULL (no data gradient in that mode),
 * else CREID_E_ARG.  creid_weight_prep_multi with CREID_BF16X3 writes the same two planes and ignores the crsk fields. */
int creid_weight_prep(const float* w_oihw, int64_t O, int64_t I, int64_t kh, int64_t kw, int dtype,
                      void* w_krsc, void* w_crsk, void* stream);
int creid_stem_weight_prep(const float* w_oihw, int dtype, void* w_stem, void* stream);
/* The same transform for MANY convolutions in one launch (LDS-tiled transposes, coalesced writes).
 * table_dev = device array of n_entries records { const float* w_oihw; void* w_krsc; void* w_crsk (nullable);
 * int32 O, I, kh, kw; int64 start } (48 bytes, creid_weight_prep_entry_bytes()); tile_start_dev = int32[n_entries]
 * = cumulative count of 32x32 (o, c) tiles, ceil(O/32)*ceil(I/32) per entry; total_tiles = their sum. */
int64_t creid_weight_prep_entry_bytes(void);
int creid_weight_prep_multi(const void* table_dev, const int32_t* tile_start_dev, int64_t n_entries,
                            int64_t total_tiles, int dtype, void* stream);
/* bf16x3 training copies, one launch over the same table (every w_crsk non-NULL): w_krsc = bf16 [2][O][r][s][I] (the forward's
 * operand, as creid_weight_prep_multi with CREID_BF16X3) and w_crsk = bf16 [2][I][r][s][O] (the data gradient's), each the hi
 * plane hi = bf16(w) then the lo plane lo = bf16(w - hi), round to nearest even.  CREID_E_ARG for a null pointer or an empty
 * table. */
int creid_weight_prep_x3_train_multi(const void* table_dev, const int32_t* tile_start_dev, int64_t n_entries,
                                     int64_t total_tiles, void* stream);

/* nn.BatchNorm2d (resnet.py:57-62,96,111; momentum 0.1, eps 1e-5) split in three steps:
 * finalize: partial (sum,sumsq) rows -> mean / invstd (+ running-stat update, unbiased variance) when
 * training, or mean = running_mean, invstd = rsqrt(running_var + eps) in eval; also emits the
 * per-channel affine scale_shift = float[2][C] {gamma*invstd, beta - mean*gamma*invstd};
 * apply: y = x * scale + shift (+ residual) (ReLU if relu) -- the fused
 * BN + residual-add + ReLU tail of Bottleneck.forward (resnet.py:72-85);
 * bwd: dy = g * [act > 0] (act nullable); dgamma += sum dy*xhat; dbeta += sum dy;
 *      dx = gamma*invstd*(dy - mean(dy) - xhat*mean(dy*xhat)); gm_out (nullable) = dy.
 *      partial = float[creid_bn2d_bwd_rows(M)][2][C] scratch (partial_ready != 0: already filled by
 *      creid_conv2d_dgrad_bnred_nhwc, the column pass is skipped), sums = float[3][C] scratch. */
int creid_bn2d_finalize(const float* partial, int64_t rows, int64_t C, int64_t count, float* running_mean,
                        float* running_var, int training, float momentum, float eps, const float* gamma,
                        const float* beta, float* mean_out, float* invstd_out, float* scale_shift,
                        void* stream);
int64_t creid_col_stats_rows(int64_t M);
int creid_col_stats(const void* x, int64_t M, int64_t C, int dtype, float* partial, void* stream);
int creid_bn2d_apply(const void* x, const float* scale_shift, const void* residual, int relu, int64_t M,
                     int64_t C, int dtype, void* y, void* stream);
/* creid_bn2d_apply that also writes the ReLU mask the backward needs as BITS: mask_out (nullable; bf16 / f16 only) =
 * uint8[M * C / 8], bit k of byte i = (y[8 i + k] > 0).  The backward then reads 1 byte per 8 channels instead of
 * re-reading y (modelling/backbones/resnet.py:71,75,85 -- the three ReLUs of a Bottleneck). */
int creid_bn2d_apply_mask(const void* x, const float* scale_shift, const void* residual, int relu, int64_t M,
                          int64_t C, int dtype, void* y, uint8_t* mask_out, void* stream);
/* Training-mode creid_bn2d_finalize + creid_bn2d_apply_mask in ONE launch (round 5), for layers with few statistic rows
 * (rows <= 1024; meant for M <= 32768): every apply workgroup sums the partial rows of its own 64-channel strip in fp64 (the
 * finalize's expressions, so mean / invstd / scale_shift / the running statistics / y / mask_out come out bit-identical to the
 * two launches), the row-block-0 workgroups publish the statistics.  count = M (the statistics cover every row of x).
 * row_blocks <= 0: chosen by the library.  C % 64 == 0 (bf16 / f16) or % 32 (f32), else CREID_E_SHAPE (use the two calls). */
int creid_bn2d_finalize_apply_mask(const float* partial, int64_t rows, int64_t C, int64_t M, float* running_mean,
                                   float* running_var, float momentum, float eps, const float* gamma, const float* beta,
                                   float* mean_out, float* invstd_out, float* scale_shift, const void* x, const void* residual,
                                   int relu, int dtype, void* y, uint8_t* mask_out, int row_blocks, void* stream);
/* bn3 + downsample BatchNorm + add + ReLU of a block with a downsample branch (resnet.py:80-85) in ONE pass:
 * y = act(x * scale + shift + (x_res * scale_res + shift_res)); x_res is the RAW downsample convolution output -- its
 * normalised tensor is never written (fp32: bit-identical to creid_bn2d_apply twice; bf16: one rounding fewer). */
int creid_bn2d_apply_dual_mask(const void* x, const float* scale_shift, const void* x_res, const float* scale_shift_res,
                               int relu, int64_t M, int64_t C, int dtype, void* y, uint8_t* mask_out, void* stream);
int64_t creid_bn2d_bwd_rows(int64_t M);
int creid_bn2d_bwd(const void* x, const void* g, const void* act, const float* mean, const float* invstd,
                   const float* gamma, int64_t M, int64_t C, int dtype, float* partial, int partial_ready,
                   float* sums, float* dgamma_accum, float* dbeta_accum, void* dx, void* gm_out, void* stream);
/* creid_bn2d_bwd with the ReLU mask as bits (mask != NULL: creid_bn2d_apply_mask's output, act is then not read). */
int creid_bn2d_bwd_mask(const void* x, const void* g, const void* act, const uint8_t* mask, const float* mean,
                        const float* invstd, const float* gamma, int64_t M, int64_t C, int dtype, float* partial,
                        int partial_ready, float* sums, float* dgamma_accum, float* dbeta_accum, void* dx,
                        void* gm_out, void* stream);
/* creid_bn2d_bwd_mask for the bn3 of a DOWNSAMPLE block (16-bit types; no act / gm_out): the pass that writes dx also produces the
 * column sums of the downsample branch's BatchNorm backward over the same masked gradient -- partial2
 * [creid_bn2d_bwd_rows(M)][2][C] from that branch's raw output x2 and its (mean2, invstd2) -- bit-identical to that layer's own
 * column pass (hand it to creid_bn2d_bwd_mask with partial_ready = 1); dx is bit-identical to creid_bn2d_bwd_mask's. */
int creid_bn2d_bwd_mask_reduce2(const void* x, const void* g, const uint8_t* mask, const float* mean, const float* invstd,
                                const float* gamma, int64_t M, int64_t C, int dtype, float* partial, int partial_ready, float* sums,
                                float* dgamma_accum, float* dbeta_accum, void* dx, const void* x2, const float* mean2,
                                const float* invstd2, float* partial2, void* stream);

/* IBN of ResNet50-IBN-a (modelling/backbones/resnet_ibn_a.py:18-32): channels [0, c_in) InstanceNorm2d
 * (affine, per-(image, channel) statistics over H*W, eps 1e-5, no running stats), channels [c_in, C)
 * BatchNorm2d; then ReLU if relu.  x, y NHWC [B*HW, C]; partial = float[B*creid_ibn_rows_per_image(HW)][2][C]
 * scratch -- or, with partial_ready = 1 and HW % 128 == 0, the (sum, sumsq) partials the producing
 * creid_conv2d_fwd_nhwc already wrote (its 128-row tiles are then whole row blocks of one image);
 * mean_out/invstd_out float[B][C]; scale_shift float[B][2][C] (saved for the backward).
 * bwd: dy = g*[act>0]; coef float[B][3][C] and per_img float[B][2][c_in] scratch; parameter
 * gradients are accumulated; partial_ready = 1: `partial` was filled by creid_conv2d_dgrad_bnred_nhwc
 * (bn_stat_image_rows = HW, HW % 128 == 0) and the column pass is skipped. */
int64_t creid_ibn_rows_per_image(int64_t HW);
int creid_ibn_fwd(const void* x, int64_t B, int64_t HW, int64_t C, int64_t c_in, const float* in_w,
                  const float* in_b, const float* bn_w, const float* bn_b, float* running_mean,
                  float* running_var, int training, float momentum, float eps, int relu, int dtype,
                  float* partial, int partial_ready, float* mean_out, float* invstd_out, float* scale_shift,
                  void* y, void* stream);
int creid_ibn_bwd(const void* x, const void* g, const void* act, const float* mean, const float* invstd,
                  int64_t B, int64_t HW, int64_t C, int64_t c_in, const float* in_w, const float* bn_w,
                  int dtype, float* partial, int partial_ready, float* coef, float* per_img, float* d_in_w,
                  float* d_in_b, float* d_bn_w, float* d_bn_b, void* dx, void* stream);
/* the same with the ReLU mask as bits (see creid_bn2d_apply_mask): mask_out / mask = uint8[B*HW*C/8], bf16 / f16 only */
int creid_ibn_fwd_mask(const void* x, int64_t B, int64_t HW, int64_t C, int64_t c_in, const float* in_w,
                       const float* in_b, const float* bn_w, const float* bn_b, float* running_mean,
                       float* running_var, int training, float momentum, float eps, int relu, int dtype,
                       float* partial, int partial_ready, float* mean_out, float* invstd_out, float* scale_shift,
                       void* y, uint8_t* mask_out, void* stream);
int creid_ibn_bwd_mask(const void* x, const void* g, const void* act, const uint8_t* mask, const float* mean,
                       const float* invstd, int64_t B, int64_t HW, int64_t C, int64_t c_in, const float* in_w,
                       const float* bn_w, int dtype, float* partial, int partial_ready, float* coef, float* per_img,
                       float* d_in_w, float* d_in_b, float* d_bn_w, float* d_bn_b, void* dx, void* stream);

/* nn.MaxPool2d(3, 2, 1) (resnet.py:98) NHWC, with the argmax tap saved for the backward (idx NULL: inference, no taps written). */
/* The stem's tail without its full-resolution intermediates (modelling/backbones/resnet.py:123-126, conv1 -> bn1 -> [relu] ->
 * maxpool): creid_bn2d_apply_maxpool3x3s2 = creid_bn2d_apply (no residual) + creid_maxpool3x3s2_fwd in one pass over the raw
 * conv output x [B, H, W, C] -- the normalised tensor is never written; y [B, H/2, W/2, C], idx as creid_maxpool3x3s2_fwd;
 * bit-identical to the two separate calls.  creid_bn2d_bwd_pooled = creid_maxpool3x3s2_bwd + creid_bn2d_bwd (no ReLU
 * mask unless act is given) with the pool gradient gathered inside the BatchNorm passes: dy_pooled [B, H/2, W/2, C] and
 * idx go in, the full-resolution gradient is never written; partial / sums as creid_bn2d_bwd; dx [B, H, W, C]. */
int creid_bn2d_apply_maxpool3x3s2(const void* x, const float* scale_shift, int relu, int64_t B, int64_t H, int64_t W,
                                  int64_t C, int dtype, void* y, uint8_t* idx, void* stream);
int creid_bn2d_bwd_pooled(const void* x, const void* dy_pooled, const uint8_t* idx, int64_t B, int64_t H, int64_t W,
                          const void* act, const float* mean, const float* invstd, const float* gamma, int64_t C,
                          int dtype, float* partial, float* sums, float* dgamma_accum, float* dbeta_accum, void* dx,
                          void* stream);
int creid_maxpool3x3s2_fwd(const void* x, int64_t B, int64_t H, int64_t W, int64_t C, int dtype, void* y,
                           uint8_t* idx, void* stream);
/* H and W even and C % 8 == 0 in all four (forward, backward and the two fused forms), else CREID_E_ARG. */
int creid_maxpool3x3s2_bwd(const void* dy, const uint8_t* idx, int64_t B, int64_t H, int64_t W, int64_t C,
                           int dtype, void* dx, void* stream);
/* nn.AdaptiveAvgPool2d(1) (modelling/baseline.py:89,93): feat fp32 [B, C]. */
int creid_gap_fwd(const void* x, int64_t B, int64_t HW, int64_t C, int dtype, float* feat, void* stream);
/* creid_gap_fwd that also adds 1 to *forward_counter (int64 on the device): the training forward's count of batches seen, folded
 * into every BatchNorm2d.num_batches_tracked before a state_dict (one counter per step instead of 53 increments). */
int creid_gap_fwd_count(const void* x, int64_t B, int64_t HW, int64_t C, int dtype, float* feat, int64_t* forward_counter,
                        void* stream);
int creid_gap_bwd(const float* dfeat, int64_t B, int64_t HW, int64_t C, int dtype, void* dx, void* stream);
/* Generalized-mean pooling with a trainable exponent, the opt-in replacement of the average pool (csrc/gem_pool.hip):
 *   u = max(x, eps), m = mean_hw u^p, feat = m^(1/p)        x [B, HW, C] in `dtype` (post-ReLU), feat fp32 [B, C].
 * p: ONE float on the device, read by the kernels (a captured training step sees the optimiser's updates); 1 <= p <= 8 is the
 * supported range, eps > 0.  The sums are formed relative to the per-(b, c) maximum, so every output is finite for every finite
 * input in that range.  C % 4 == 0 for CREID_F32 and C % 8 == 0 for the 16-bit types, any HW >= 1, B <= 65535; NULL x / p /
 * feat, a C off the vector width or eps <= 0 return CREID_E_ARG and any other dtype CREID_E_DTYPE before anything is launched.
 * creid_gem_fwd: stats (optional, fp32 [3][B][C]) receives what the backward needs per (b, c): the maximum, the coefficient
 * of dx and dfeat's coefficient in dp; NULL (eval) skips them.  forward_counter (optional, int64 on the device): += 1, as
 * creid_gap_fwd_count.
 * creid_gem_bwd: one pass over the saved map x: dx [B, HW, C] in `dtype` = dfeat * (1/HW) * m^(1/p - 1) * u^(p - 1) where
 * x >= eps and a true zero below (the gradient of clamp(min = eps)); a loss scale carried by dfeat is carried by dx and dp.
 * p_grad (optional, ONE float): += dp, summed deterministically -- one partial per workgroup into partials
 * (creid_gem_bwd_partials(B, C, dtype) floats, required with p_grad), then a fixed-order sum in a second, one-workgroup launch;
 * no floating-point atomics, two calls give the same bits. */
int64_t creid_gem_bwd_partials(int64_t B, int64_t C, int dtype);
int creid_gem_fwd(const void* x, int64_t B, int64_t HW, int64_t C, int dtype, const float* p, float eps, float* feat,
                  float* stats, int64_t* forward_counter, void* stream);
int creid_gem_bwd(const void* x, const float* dfeat, const float* stats, int64_t B, int64_t HW, int64_t C, int dtype,
                  const float* p, float eps, void* dx, float* p_grad, float* partials, void* stream);
/* NHWC compute dtype -> NCHW fp32 (to return `base_out` in the reference's layout). */
int creid_nhwc_to_nchw_f32(const void* x, int64_t B, int64_t HW, int64_t C, int dtype, float* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CREID_H */
