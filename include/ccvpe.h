/*
 * ccvpe.h - C ABI of libccvpe_hip.so: the MI355X (gfx950) inference forward pass of CCVPE.
 *
 * The reference is pure Python/PyTorch and has no native interface of its own; the hot path it
 * exposes is `CVM_*.forward(grd, sat)` (reference models.py:150, 448, 752, 1051) on an nn.Module
 * whose parameters arrive through `load_state_dict` (reference train_VIGOR.py:248-254).  This
 * header is what a binding for that path binds:
 *
 *   reference interface                                   replaced by
 *   ----------------------------------------------------  -----------------------------------------
 *   CVM_VIGOR(device, circular_padding)        models.py:50    ccvpe_create (variant 0)
 *   CVM_VIGOR_ori_prior(device, ori_noise, circ) models.py:347 ccvpe_create (variant 1)
 *   CVM_KITTI(device)                          models.py:656   ccvpe_create (variant 2)
 *   CVM_OxfordRobotCar(device)                 models.py:955   ccvpe_create (variant 3)
 *   load_state_dict(state_dict)          train_VIGOR.py:252    ccvpe_set_weight x818 + ccvpe_finalize_weights
 *   forward(grd, sat) -> 9-tuple   models.py:150,448,752,1051  ccvpe_forward
 *   per-sample argmax / (cos,sin) lookup train_VIGOR.py:297-316 ccvpe_postprocess
 *
 * Conventions
 *   - all tensors are float32; inputs/outputs are NCHW-contiguous exactly as the reference's
 *     forward receives and returns them; pointers are DEVICE pointers borrowed from the caller
 *     (e.g. torch.Tensor.data_ptr()) and are never freed or retained by the library;
 *   - every function returns 0 on success or a negative CCVPE_E* code; ccvpe_last_error() gives
 *     a thread-local human-readable message; nothing throws across the ABI;
 *   - a handle is bound to one HIP device and is not re-entrant; launches go to the caller's
 *     stream, asynchronously, with no hidden synchronisation once the plan for a given
 *     (batch, ground size) exists (the first call with a new shape allocates workspace);
 *   - there is no CPU fallback: without a gfx950 device every compute entry point fails.
 */
#ifndef CCVPE_H
#define CCVPE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCVPE_OK 0
#define CCVPE_EINVAL (-1)   /* bad argument / shape */
#define CCVPE_ESTATE (-2)   /* call order (e.g. forward before finalize) */
#define CCVPE_EHIP (-3)     /* HIP runtime error */
#define CCVPE_ENOMEM (-4)
#define CCVPE_EKEY (-5)     /* unknown / missing state_dict key */

#define CCVPE_VARIANT_VIGOR 0
#define CCVPE_VARIANT_VIGOR_ORI_PRIOR 1
#define CCVPE_VARIANT_KITTI 2
#define CCVPE_VARIANT_OXFORD 3

#define CCVPE_OUT_HW 512       /* localisation / orientation maps are 512 x 512 (models.py:319-341) */
#define CCVPE_SAT_HW 512       /* aerial input is 3 x 512 x 512 */

typedef struct ccvpe_handle_s* ccvpe_handle;

typedef struct ccvpe_config {
    int32_t variant;            /* CCVPE_VARIANT_* */
    int32_t circular_padding;   /* ground encoder: horizontal circular padding (models.py:53, utils.py:330-358) */
    float   ori_noise;          /* variant 1 only: rolls i = -n..n, n = int(ori_noise/18) (models.py:489) */
    int32_t device;             /* HIP device ordinal */
    int32_t micro_batch;        /* samples per internal pass (0 = library default); larger batches loop */
    int32_t reserved[3];        /* reserved[0] = precision mode of the dense contractions:
                                   0 exact fp32 MFMA (default); 1 "bf16x3": fp32 operands split into two bf16,
                                   three bf16 MFMAs per product, fp32 accumulate (~2^-16 relative per term) */
} ccvpe_config;

/* Caller-allocated outputs of one forward call (device memory, NCHW contiguous, batch-major).
 * Channel counts of ms[k] come from ccvpe_output_channels(). */
typedef struct ccvpe_outputs {
    float* logits_flattened;    /* [B, 512*512]                                  models.py:319 */
    float* heatmap;             /* [B, 1, 512, 512] softmax over all pixels       models.py:320 */
    float* ori;                 /* [B, 2, 512, 512] unit (cos, sin) field         models.py:341 */
    float* matching_score[6];   /* level k: [B, R_k, 8*2^k, 8*2^k], k = 0..5      models.py:343 */
} ccvpe_outputs;

/* Compact per-sample result of the test-loop post-processing (train_VIGOR.py:297-316). */
typedef struct ccvpe_pose {
    int32_t index;              /* argmax of the heatmap, y*512 + x; -1: the map holds no value above -inf (below) */
    float   prob;               /* heatmap value there; NaN for index -1 */
    float   cos_v, sin_v;       /* orientation field at that pixel; at pixel 0 for index -1 */
    float   angle_deg;          /* acos/sign rule of train_VIGOR.py:307-311, in [0, 360) */
} ccvpe_pose;

/* Per-query evaluation record of the reference test loops (train_VIGOR.py:296-326, train_KITTI.py:309-343), double
 * precision like their numpy / math arithmetic.  NaN = the reference does not produce that number for the query. */
typedef struct ccvpe_metrics {
    double pixel_distance;         /* |argmax(gt) - argmax(heatmap)| in output pixels          train_VIGOR.py:299 */
    double meter_distance;         /* pixel_distance * meter_per_pixel[b]                       :301-309 */
    double prob_at_gt;             /* heatmap at the ground-truth pixel                         :326 */
    double angle_pred_deg;         /* acos / sign rule on the predicted (cos, sin)              :306-311 */
    double angle_gt_deg;           /* the same on the ground-truth (cos, sin)                   :312-317 */
    double orientation_error_deg;  /* min(|gt - pred|, 360 - |gt - pred|)                       :319 */
    double longitudinal_m;         /* KITTI / Oxford: error along the driving direction         train_KITTI.py:322-324 */
    double lateral_m;              /* ... and across it                                          train_KITTI.py:323-325 */
} ccvpe_metrics;

const char* ccvpe_last_error(void);
const char* ccvpe_version(void);
/* Kernel launches this THREAD has issued through the library so far (every entry point; eager launches - a replayed hipGraph issues
 * none).  The difference around a call = its launches: bench.py's `launches_per_frame`.  No reference counterpart. */
uint64_t ccvpe_launch_count(void);

int ccvpe_create(const ccvpe_config* cfg, ccvpe_handle* out);
int ccvpe_destroy(ccvpe_handle h);

/* One state_dict entry.  `data` may be a host or a device pointer (float32, contiguous, `shape`
 * as in the reference state_dict); BatchNorm `num_batches_tracked` (int64) entries and the unused
 * `_fc.*` classifier are accepted and ignored via ccvpe_skip_weight.  Returns CCVPE_EKEY for a key
 * that is not part of the 818-key layout, CCVPE_EINVAL for a shape mismatch. */
int ccvpe_set_weight(ccvpe_handle h, const char* key, const float* data, const int64_t* shape, int32_t ndim);
int ccvpe_skip_weight(ccvpe_handle h, const char* key);
/* Folds BatchNorm into the adjacent convolutions, repacks everything into the kernels' layouts and
 * uploads it.  Fails with CCVPE_EKEY (message lists the first missing key) if any key is unset. */
int ccvpe_finalize_weights(ccvpe_handle h);

/* Packed-weight cache (reference train_VIGOR.py:252 reloads and, here, re-packs the checkpoint on every start): after
 * ccvpe_finalize_weights, ccvpe_save_packed writes the folded / repacked / Winograd-transformed device weights to `path`;
 * in a later process ccvpe_load_packed(h, path) on a handle created with the same config replaces the 818 ccvpe_set_weight
 * calls and ccvpe_finalize_weights.  The caller keys the file by the checkpoint's content (see ccvpe_amd/models.py).
 * CCVPE_EINVAL if the file is missing, truncated, or was packed for another variant / precision / library build or under other
 * packer switches than the loading handle's (ccvpe_pack_switches). */
int ccvpe_save_packed(ccvpe_handle h, const char* path);
int ccvpe_load_packed(ccvpe_handle h, const char* path);
/* The environment switches that change what the packer emits and differ from their defaults, as "NAME=value;" pairs in a fixed
 * order ("" when none does; thread-local storage, valid until the thread's next call): part of the caller's cache key, so a file
 * packed under one setting is never loaded under another.  Read from the environment at the call, as ccvpe_create reads it for a
 * handle.  No reference counterpart. */
const char* ccvpe_pack_switches(void);

/* Tuning table.  The first forward of a new (batch, ground size) measures every tiled launch of its plan with each candidate
 * kernel tile and keeps the fastest (1-2 s at batch 32); the choices are the only thing about a forward that can differ between
 * two processes.  ccvpe_export_tuning writes them as text (one "op <launch key> <tile name> <split>" line per launch; call with
 * buf = NULL to get the size in *needed), ccvpe_import_tuning loads such text (returns the number of entries read): a launch
 * found in the table is not measured again and runs exactly as recorded, so two handles with the same table produce
 * bit-identical results.  ccvpe_tuning_generation counts the plans this handle has measured launches of (the host side saves
 * the table when it grows; see ccvpe_amd/tuning.py).  No reference counterpart. */
int ccvpe_import_tuning(ccvpe_handle h, const char* text);
int ccvpe_export_tuning(ccvpe_handle h, char* buf, size_t capacity, size_t* needed);
int ccvpe_tuning_generation(ccvpe_handle h);

/* Largest micro_batch whose intermediate tensors all stay below the 2 GiB the kernels address with 32-bit byte offsets
 * (ccvpe_forward refuses a larger one with CCVPE_EINVAL instead of wrapping offsets).  Pure host arithmetic, no device
 * needed.  Negative on a ground size the variant's descriptor heads cannot take.  It has no handle and so plans for zero
 * padding: for widths 32..63 it returns a positive batch although a handle created with circular_padding = 1 refuses them
 * (ccvpe_forward and ccvpe_workspace_bytes of that handle decide). */
int ccvpe_max_micro_batch(int32_t variant, float ori_noise, int32_t grd_h, int32_t grd_w);

/* R_k of matching_score[level] (level 0..5) for this handle's variant / ori_noise. */
int ccvpe_output_channels(ccvpe_handle h, int32_t level);
/* Device workspace the library holds for a (batch, ground size) plan, in bytes (0 on error). */
size_t ccvpe_workspace_bytes(ccvpe_handle h, int32_t batch, int32_t grd_h, int32_t grd_w);

/* forward(grd, sat): grd [B,3,grd_h,grd_w], sat [B,3,512,512], device pointers, NCHW float32.
 * `stream` is a hipStream_t (NULL = default stream). */
int ccvpe_forward(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const float* sat,
                  int32_t batch, const ccvpe_outputs* out, void* stream);

/* Device-side test-loop post-processing on forward outputs: poses[B] is DEVICE memory.  batch <= 4096 per call; one call in flight per
 * handle (the launch keeps per-sample partial results and ticket counters in a scratch buffer of the handle).
 * The argmax: the largest value above -inf, the first index on ties; NaN compares false and never wins, unlike
 * numpy.argmax, which returns the first NaN.  A map without a value above -inf (all NaN - what the softmax makes of one NaN or +inf
 * logit -, all -inf, a mix) has no argmax: index -1, prob NaN, and cos / sin / angle of pixel 0.  Nothing is read outside the maps. */
int ccvpe_postprocess(ccvpe_handle h, const float* heatmap, const float* ori, int32_t batch,
                      ccvpe_pose* poses, void* stream);
/* The same five numbers per query as one float row - rows[B][5] = (index, prob, cos, sin, angle_deg), DEVICE memory: the 20-byte
 * record a data-parallel evaluation gathers (train_VIGOR.py:297-316 keeps them in Python lists).  batch <= 4096. */
int ccvpe_postprocess_rows(ccvpe_handle h, const float* heatmap, const float* ori, int32_t batch,
                           float* rows, void* stream);
/* The K strongest pose hypotheses per query instead of the argmax alone: rows[B][k][5] = (index, prob, cos, sin, angle_deg),
 * DEVICE memory, the row layout of ccvpe_postprocess_rows.  Pixel q suppresses pixel p when q != p, max(|qy-py|, |qx-px|) <=
 * radius and heatmap[q] > heatmap[p], or the two are equal and q < p (NaN never suppresses); p is a peak when heatmap[p] > 0
 * and nothing suppresses it.  Peaks are ordered by value (descending), then index (ascending); a query with fewer than k
 * peaks gets rows (-1, 0, 0, 0, 0) for the rest.  k = 1 on a map without NaN gives the ccvpe_postprocess_rows row.
 * k 1..64, radius 0..32, batch <= 4096; CCVPE_EINVAL for a null pointer or an argument out of range (checked before the
 * handle is used).  One call in flight per handle, as ccvpe_postprocess (the launch keeps ticket counters and per-tile
 * candidates in a scratch buffer of the handle). */
int ccvpe_postprocess_topk(ccvpe_handle h, const float* heatmap, const float* ori, int32_t batch, int32_t k,
                           int32_t radius, float* rows, void* stream);

/* Ground-truth side of the same test loop, on device: `poses` from ccvpe_postprocess, `gt_index[B]` = flat index of
 * argmax(gt map) (y*512 + x), `gt_cos_sin[B][2]` = ground-truth orientation at that pixel (NULL: no orientation error),
 * `meter_per_pixel[B]` = metres per OUTPUT pixel (VIGOR: city constant / 512 * 640, train_VIGOR.py:301-308; KITTI:
 * test_set.meter_per_pixel), `heading_deg[B]` = orientation_angle of train_KITTI.py:310 (NULL: no lateral / longitudinal
 * split).  All pointers are DEVICE memory; out[B] likewise.  A pose with index < 0 (no argmax) gives NaN distances (pixel, metre,
 * longitudinal, lateral); a gt_index outside [0, 512*512) gives prob_at_gt = NaN and the heatmap is not read there. */
int ccvpe_eval_metrics(ccvpe_handle h, const ccvpe_pose* poses, const float* heatmap, int32_t batch, const int32_t* gt_index,
                       const float* gt_cos_sin, const double* meter_per_pixel, const double* heading_deg, ccvpe_metrics* out,
                       void* stream);

/* Aerial-side caching for streaming (reference datasets.py:306-317 reuses aerial tiles across frames, the
 * reference model still re-encodes them every call): encode once, then run ground encoder + matching +
 * decoders against the cached aerial encoding.  `cache` is caller-owned DEVICE memory of
 * ccvpe_aerial_cache_bytes(h, batch) bytes; batch <= micro_batch.  forward_cached(grd, encode(sat)) ==
 * forward(grd, sat). */
size_t ccvpe_aerial_cache_bytes(ccvpe_handle h, int32_t batch);
int ccvpe_encode_aerial(ccvpe_handle h, const float* sat, int32_t batch, void* cache, void* stream);
int ccvpe_forward_cached(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const void* cache,
                         int32_t batch, const ccvpe_outputs* out, void* stream);

/* Pose-only forward: rows[B][5] = (index, prob, cos, sin, angle_deg), DEVICE memory, bit-identical to
 * ccvpe_forward + ccvpe_postprocess_rows on the same inputs, without writing the nine forward outputs (no heatmap, no
 * matching-score stacks; the orientation field is computed only around each sample's argmax).  Arguments as ccvpe_forward;
 * larger batches than the micro-batch loop the same way.  A query whose softmax statistics are not finite (a NaN or +inf logit,
 * -inf everywhere: the forward's heatmap is then all NaN) gets ccvpe_postprocess_rows' row for such a map, (-1, NaN, cos / sin /
 * angle of pixel 0), as the prior, tracking, summary and heading forms do.  CCVPE_EINVAL for a null `rows`, CCVPE_ESTATE on a handle with debug
 * taps on (ccvpe_set_debug).  Pose plans run eagerly, never as a captured hipGraph (CCVPE_GRAPH=1 included). */
int ccvpe_localize(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const float* sat,
                   int32_t batch, float* rows, void* stream);
/* The same with the aerial side from ccvpe_encode_aerial (batch <= micro_batch, as ccvpe_forward_cached). */
int ccvpe_localize_cached(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const void* cache,
                          int32_t batch, float* rows, void* stream);
/* Pose-only forward with the K strongest hypotheses per query: rows[B][k][5], DEVICE memory, bit-identical to ccvpe_forward +
 * ccvpe_postprocess_topk(k, radius) on the same inputs, without writing the nine forward outputs (the orientation field is
 * computed only around each hypothesis).  Restrictions as ccvpe_localize (micro-batch loop, CCVPE_ESTATE on a debug handle,
 * never a captured hipGraph); CCVPE_EINVAL for a null pointer, k outside 1..64 or radius outside 0..32, checked before the
 * handle is used.  Every (k, radius) runs the same plan. */
int ccvpe_localize_topk(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const float* sat,
                        int32_t batch, int32_t k, int32_t radius, float* rows, void* stream);
/* The same with the aerial side from ccvpe_encode_aerial (batch <= micro_batch, as ccvpe_forward_cached). */
int ccvpe_localize_topk_cached(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const void* cache,
                               int32_t batch, int32_t k, int32_t radius, float* rows, void* stream);

/* Indexed cached forms: a batch of queries against a few shared tiles (the Oxford test split crops its aerial window on a
 * 400-px grid, so consecutive frames share tiles).  `cache` was written by ccvpe_encode_aerial(h, sat, n_tiles, cache, ...),
 * 1 <= n_tiles <= micro_batch; query b is paired with tile tile_index[b].  `tile_index` is HOST memory, int32 [batch], every
 * entry in 0 .. n_tiles-1.  `batch` is any positive count: larger batches loop over micro-batches as ccvpe_forward does, each
 * slice reading its own entries of tile_index from the same cache.  Outputs and rows are laid out as in ccvpe_forward_cached,
 * ccvpe_localize_cached and ccvpe_localize_topk_cached; with n_tiles == batch and tile_index[b] == b the results are
 * bit-identical to those calls.  CCVPE_EINVAL, with no launch issued, for a null pointer, n_tiles <= 0, an index out of range
 * (the message names the first bad position and value) or, for the top-K form, k / radius out of range - all checked before
 * the handle is used - and for n_tiles > micro_batch.  The indices travel in the launch arguments: no copy to the device,
 * no synchronisation, and the caller may reuse tile_index as soon as the call returns. */
int ccvpe_forward_cached_indexed(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const void* cache,
                                 int32_t n_tiles, const int32_t* tile_index, int32_t batch, const ccvpe_outputs* out,
                                 void* stream);
int ccvpe_localize_cached_indexed(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const void* cache,
                                  int32_t n_tiles, const int32_t* tile_index, int32_t batch, float* rows, void* stream);
int ccvpe_localize_topk_cached_indexed(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const void* cache,
                                       int32_t n_tiles, const int32_t* tile_index, int32_t batch, int32_t k, int32_t radius,
                                       float* rows, void* stream);

/* Ground-side cache: the descriptor vector of each ground image, the ground encoder's only output.  Layout: float32
 * [batch][Ltot], DEVICE memory of ccvpe_ground_cache_bytes(h, batch, grd_h, grd_w) = batch * Ltot * 4 bytes, where
 * Ltot = sum over the six matching levels k of round_up(L_k, 4), L_k = (feature width) * (head channels of level k), and level
 * k's descriptor starts at float sum_{j<k} round_up(L_j, 4) of its row; the round_up(L_k, 4) - L_k padding floats behind a level are
 * written as 0 by every call, whatever the buffer held.  batch <= micro_batch.
 * The launches are the full forward's ground encoder, heads and descriptor launch: at the same batch the cache holds the bits
 * the full forward computes.  ccvpe_ground_cache_bytes returns 0 for a bad argument or ground geometry (ccvpe_last_error). */
size_t ccvpe_ground_cache_bytes(ccvpe_handle h, int32_t batch, int32_t grd_h, int32_t grd_w);
int ccvpe_encode_ground(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, int32_t batch, void* cache,
                        void* stream);

/* One ground encoding per query against several aerial tiles (VIGOR's positive and semi-positive tiles, Oxford's overlapping
 * 400-px windows, a coarse position prior).  `grd_cache` is ccvpe_encode_ground's cache of n_queries images of grd_h x grd_w,
 * `sat_cache` ccvpe_encode_aerial's cache of n_tiles tiles.  The pairs form a CSR list in HOST memory: query g owns pairs
 * offsets[g] .. offsets[g+1]-1 (offsets: int32 [n_queries+1]), pair p uses tile tiles[p] (int32 [P], P = offsets[n_queries]);
 * a tile may appear several times, each a pair of its own.  P is any count: the pairs run as micro-batches of the cached pose
 * plan, every pair reading its query's row and its tile from the two caches.  DEVICE outputs, all required:
 *   pair_rows[P][5]   ccvpe_localize rows of each pair, the probability normalised inside that pair's tile;
 *   pair_stats[P][2]  (m_p, inv_p) = (max logit, 1 / sum exp(logit - m_p)) of that tile's softmax;
 *   tile_prob[P]      S_p / Z with S_p = exp(m_p - M) / inv_p, M the query's largest m_p, Z the sum of its S_p: the pair's share of
 *                     the query's summed softmax mass (tiles overlap: not a posterior over disjoint areas);
 *   rows[n_queries][5] the row of the query's best pair with prob = joint_p = prob_p * S_p / Z, the softmax over the union of the
 *                     query's tiles at that pair's argmax; the best pair has the largest joint_p, the first on ties;
 *   best_pair[n_queries] that pair's position p.
 * The cross-tile step is float64.  A pair whose m_p or inv_p is not finite has S_p = 0 and never wins; a query without a finite
 * pair reports its first pair with prob NaN (and NaN tile_prob).  CCVPE_EINVAL, with no launch issued and every output
 * untouched, checked before the handle is used: a null pointer, n_queries <= 0, n_tiles <= 0, offsets[0] != 0, offsets that do
 * not strictly increase (a query without a tile), a tile outside 0 .. n_tiles-1 (the message names the first bad position and
 * value); then n_queries or n_tiles > micro_batch.  CCVPE_ESTATE on a debug handle.  The CSR arrays travel in the launch
 * arguments: no copy to the device, no synchronisation, and the caller may reuse them as soon as the call returns. */
int ccvpe_localize_region(ccvpe_handle h, const void* grd_cache, int32_t n_queries, int32_t grd_h, int32_t grd_w,
                          const void* sat_cache, int32_t n_tiles, const int32_t* offsets, const int32_t* tiles,
                          float* rows, int32_t* best_pair, float* pair_rows, float* pair_stats, float* tile_prob,
                          void* stream);

/* Localize with a per-query position prior (a GNSS fix, the previous pose plus odometry, a road mask).  `log_prior` is float32
 * DEVICE memory in the output-map frame, 512 x 512 values per map in the pixel order of logits_flattened: log-weights, not
 * necessarily normalised, -inf excluding a pixel.  prior_stride (in floats) is 0 (one map for every query) or 512*512 (one map
 * per query); larger batches than micro_batch read each slice's own maps.  With l the logits the plan computes, per query:
 *     l' = fl32(l + log_prior)                  one IEEE float add per pixel
 *     (m', inv') = max of l' and 1 / sum exp(l' - m'), the library's softmax statistics (the same order of combines)
 *     h' = __expf(l' - m') * inv'               the heatmap expression of ccvpe_forward
 * k == 0 (radius 0): rows[B][5] = (index, prob, cos, sin, angle_deg) at the first maximal h', prob = h' there, the orientation
 * field at that pixel, as ccvpe_localize.  k in 1..64, radius in 0..32: rows[B][k][5] with ccvpe_postprocess_topk's peaks,
 * order and (-1, 0, 0, 0, 0) padding applied to h'.  A query without a finite posterior (m' or inv' not finite: a prior of -inf
 * over the whole map, a +inf or a NaN anywhere) has the argmax row (-1, NaN, cos / sin / angle of pixel 0) and top-K rows all
 * (-1, 0, 0, 0, 0); no launch reads outside its tensors whatever the prior holds.  An all-zero prior gives the bits of the
 * forms without a prior (logits without NaN or inf).  No launch is added: the prior is read where the logits are.
 * CCVPE_EINVAL, with nothing launched and checked before the handle is used: a null pointer, prior_stride other than 0 or
 * 512*512, k outside 0..64, radius outside 0..32, radius != 0 with k == 0 (the message names the argument); then the checks of
 * the forms without a prior.  CCVPE_ESTATE on a debug handle (the three localize forms). */
int ccvpe_localize_prior(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const float* sat, int32_t batch,
                         const float* log_prior, int64_t prior_stride, int32_t k, int32_t radius, float* rows, void* stream);
/* The cached form: tile_index (HOST int32 [batch], as ccvpe_localize_cached_indexed) or NULL, query b then reading tile b of a
 * cache of n_tiles == batch tiles (the plan of ccvpe_localize_cached). */
int ccvpe_localize_prior_cached_indexed(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const void* cache,
                                        int32_t n_tiles, const int32_t* tile_index, int32_t batch, const float* log_prior,
                                        int64_t prior_stride, int32_t k, int32_t radius, float* rows, void* stream);
/* The same rows from forward outputs the caller holds: `logits` is ccvpe_forward's logits_flattened [batch][512*512], `ori` its
 * orientation field [batch][2][512][512].  Bit-identical to the pose-only forms on the same inputs.  batch <= 4096; any
 * handle (debug included); one call in flight per handle (ticket counters and partials in a scratch buffer of the handle). */
int ccvpe_postprocess_prior(ccvpe_handle h, const float* logits, const float* ori, int32_t batch, const float* log_prior,
                            int64_t prior_stride, int32_t k, int32_t radius, float* rows, void* stream);
/* ccvpe_localize_region with a prior per pair: pair p reads the map at pair_log_prior + p * prior_stride (stride 0: one map for
 * every pair).  pair_rows are the k == 0 rows of each pair's posterior and pair_stats its (m', inv'); the cross-tile step is
 * ccvpe_localize_region's on them, so a pair without a finite posterior never wins.  The maps of one query's tiles must share
 * one scale - a log-density evaluated at each heatmap pixel's map position, not a map normalised inside each tile - or tile_prob
 * and the joint probability compare nothing.  Argument checks: ccvpe_localize_region's, then a null pair_log_prior or a bad
 * prior_stride. */
int ccvpe_localize_region_prior(ccvpe_handle h, const void* grd_cache, int32_t n_queries, int32_t grd_h, int32_t grd_w,
                                const void* sat_cache, int32_t n_tiles, const int32_t* offsets, const int32_t* tiles,
                                const float* pair_log_prior, int64_t prior_stride, float* rows, int32_t* best_pair,
                                float* pair_rows, float* pair_stats, float* tile_prob, void* stream);

/* Tracking a frame stream: a recursive Bayes (histogram) filter over the 512 x 512 position grid, one step per frame =
 * ccvpe_track_predict (the previous posterior -> this frame's log-prior) + ccvpe_track_update* (this frame's posterior).
 *
 * Update.  rows [batch][5] are exactly the k == 0 rows of ccvpe_localize_prior / ccvpe_localize_prior_cached_indexed /
 * ccvpe_postprocess_prior for the same arguments.  `posterior` is float32 DEVICE memory [batch][512*512] in the pixel order of
 * logits_flattened and receives h' = __expf(l' - m') * inv' of the definition above - the bits rows[b][1] carries at
 * rows[b][0].  log_prior may be NULL (prior_stride is then ignored): l' = l and the map is ccvpe_forward's heatmap.  A query
 * without a finite posterior keeps the row (-1, NaN, ...) and gets an all-zero map, so that with a positive floor the next
 * predicted prior is flat and the filter starts over instead of spreading NaN.  No launch is added to the pose plans: the map
 * is stored by the launch that finds the argmax.  CCVPE_EINVAL, nothing launched, checked before the handle is used: the
 * checks of the matching prior form (a null log_prior excepted), a null posterior, a posterior that is log_prior or logits. */
int ccvpe_track_update(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const float* sat, int32_t batch,
                       const float* log_prior, int64_t prior_stride, float* rows, float* posterior, void* stream);
int ccvpe_track_update_cached_indexed(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const void* cache,
                                      int32_t n_tiles, const int32_t* tile_index, int32_t batch, const float* log_prior,
                                      int64_t prior_stride, float* rows, float* posterior, void* stream);
int ccvpe_track_update_logits(ccvpe_handle h, const float* logits, const float* ori, int32_t batch, const float* log_prior,
                              int64_t prior_stride, float* rows, float* posterior, void* stream);
/* Predict.  All pointers DEVICE float32: belief [batch][512*512] (a posterior map), shift [batch][2] = (dx, dy) in output
 * pixels, taps the one-sided blur weights t[0..radius] (taps_stride 0: one set for every query; radius + 1: one per query),
 * radius 0..32, floor [batch] >= 0, log_prior [batch][512*512] out (must not alias belief).  Per query, with the belief extended
 * by zero outside its grid, on the infinite plane
 *     s(x, y)   = bilinear sample of the belief at (x - dx, y - dy)             the content moves by (+dx, +dy)
 *     c         = s convolved with t[|i|], i = -radius..radius, along x, then along y
 *     out(x, y) = logf(c(x, y) + floor)                                          for the 512 x 512 window only
 * Mass that leaves the window is lost; floor stands for it (and for a relocalisation probability).  floor = 0 and c = 0 give
 * -inf, which the prior forms read as "pixel excluded".  A fractional part of exactly 0 weighs the one source pixel with
 * exactly 1.  The bilinear weights are folded into the two passes (every term is non-negative; a pass is 2 radius + 2 fused
 * multiply-adds), so c is within a relative (4 radius + 12) * 2^-24 of the exact value.  NaN / inf shifts may give NaN, but no
 * launch reads outside its tensors whatever the inputs hold.  One launch.  CCVPE_EINVAL, nothing launched, checked before the
 * handle is used: a null pointer, radius outside 0..32, a taps_stride other than 0 or radius + 1, batch outside 1..4096,
 * log_prior == belief. */
int ccvpe_track_predict(ccvpe_handle h, const float* belief, int32_t batch, const float* shift, const float* taps,
                        int32_t taps_stride, int32_t radius, const float* floor, float* log_prior, void* stream);
/* Predict under an affine map: the belief of a frame whose grid is a rotated, rescaled or sheared view of this frame's (KITTI's
 * heading-up tiles, a zoom change).  matrix is float64 DEVICE memory [batch][6], M = (m0..m5) per query; the other arguments are
 * ccvpe_track_predict's.  M maps an OUTPUT pixel to the SOURCE position it reads - the direction of Pillow's AFFINE data and of
 * ccvpe_preprocess_affine - but in INDEX coordinates: belief[j][i] sits at position (i, j), not at Pillow's pixel centre
 * (i + 0.5, j + 0.5).  Per query, with the belief extended by zero outside its grid, on the infinite plane, for integer x, y
 *     (sx, sy)  = (m0 x + m1 y + m2, m3 x + m4 y + m5)                          float64
 *     s(x, y)   = |m0 m4 - m1 m3| * bilinear sample of the belief at (sx, sy)
 *     c         = s convolved with t[|i|], i = -radius..radius, along x, then along y
 *     out(x, y) = logf(c(x, y) + floor)                                          for the 512 x 512 window only
 * ccvpe_track_predict is the case M = (1, 0, -dx, 0, 1, -dy), and for integer dx, dy the two give the same bits.  |det|, rounded
 * once to float32, keeps the mass of a belief that stays inside the window when the map changes scale; det = 0 gives logf(floor)
 * everywhere.  Arithmetic: coordinates float64; ix = floor(sx); the fraction (float)(sx - ix) is rounded once to float32, the
 * weights are 1.f - f and f, the sample is a float32 sum of non-negative terms, a fraction of exactly 0 weighs the one source
 * pixel with exactly 1; a pass is 2 radius + 1 fused multiply-adds.  c is within (4 radius + 12) * 2^-24 * c + 2^-38 * max(belief)
 * of the exact value: the first term counts the roundings of non-negative terms, the second covers what a coordinate rounding of
 * 2^-42 px can move a sample by (for |det| <= 4 and positions within +-1024).  Non-finite matrix entries may give NaN, but no launch reads outside its tensors whatever the
 * inputs hold: the integer parts are clamped to +-2048 (NaN included) before they are converted and every read is checked against
 * the grid.  One launch; a pure translation is NOT re-routed to ccvpe_track_predict.  CCVPE_EINVAL as ccvpe_track_predict (a null
 * matrix for a null shift). */
int ccvpe_track_predict_affine(ccvpe_handle h, const float* belief, int32_t batch, const double* matrix, const float* taps,
                               int32_t taps_stride, int32_t radius, const float* floor, float* log_prior, void* stream);

/* Smoothing a tracked stream: the backward half of the histogram filter.  The filter answers p(x_t | frames 1..t); one call of
 * ccvpe_track_smooth per frame, from the last frame back, turns the stored beliefs into p(x_t | frames 1..T).  All map pointers
 * DEVICE float32 [batch][512*512]: `belief` the filter posterior of frame t (ccvpe_track_update's map), `smoothed_next` the
 * smoothed map of frame t + 1 (for the last frame but one: the last frame's own belief), `smoothed` out.  shift, taps,
 * taps_stride, radius, floor: the arguments of the ccvpe_track_predict call that carried `belief` into frame t + 1.  With
 * P(m; dx, dy) that call's c for a map m (zero extension, bilinear shift, x pass then y pass, the window only), per query
 *     prior_i = P(belief; dx, dy)_i + floor            the bits ccvpe_track_predict takes the logf of
 *     g_i     = s'_i > 0 ? s'_i / prior_i : 0          (s' = smoothed_next; NaN and negative s' are not taken)
 *     G       = sum_i g_i
 *     a_i     = fma(floor, G, P(g; -dx, -dy)_i)        P with the negated shift is the adjoint of P
 *     w_i     = belief_i * a_i,   Z = sum_i w_i,   smoothed_i = w_i * (1 / Z)
 * which inverts the transition T(x'|x) = u(x' - x - d) + floor of the filter's predict; Z = sum s' (1 up to rounding) when the
 * belief has mass 1.  stats [batch][4] = (index, prob, Z, G): index the first index of the largest w, as float; prob the bits
 * of smoothed[index].
 *   - G == 0 (the next map has no positive cell - the zero map of a frame without a finite posterior, a broken link): the
 *     future says nothing, smoothed is belief bit for bit, index / prob its argmax (a value is taken when it is above -inf,
 *     NaN never wins, the first index wins ties; no taken value: -1, NaN), Z = NaN, G = 0.
 *   - else Z not finite or Z <= 0 (a zero belief, a NaN in belief, floor = 0 and prior_i = 0 under a positive s'_i): an
 *     all-zero map and (-1, NaN, Z, G).
 * Queries are independent: a poisoned query changes no bit of its neighbours.  No launch reads outside its tensors whatever
 * the inputs hold (ccvpe_track_predict's clamps and guards).  Every sum has a fixed order and nothing is accumulated
 * atomically: the same inputs give the same bits on every call, alone as in a batch.  Relative error of smoothed against the
 * exact recursion on the same float32 inputs: at most (16 radius + 97) * 2^-24 to first order.
 * `work` is DEVICE memory of ccvpe_track_smooth_work_bytes(batch) bytes (pure host arithmetic; 0 for batch <= 0), 16-byte
 * aligned, any contents: it holds g and the per-tile partial sums between the launches, and nothing in it has to survive a
 * call.  The call allocates nothing, synchronises nothing and uses no scratch of the handle: calls on several streams of one
 * handle may run at once when each has its own work, smoothed and stats.  `smoothed` may be `smoothed_next`: a backward sweep
 * can run in one buffer, with the bits of the out-of-place call.  Three launches.  CCVPE_EINVAL, nothing launched, checked
 * before the handle is used: a null pointer, radius outside 0..32, a taps_stride other than 0 or radius + 1, batch outside
 * 1..4096, smoothed or stats equal to belief, work or each other, smoothed_next == belief, a map or work that is not 16-byte
 * aligned (the kernels read and write the maps four cells at a time). */
size_t ccvpe_track_smooth_work_bytes(int32_t batch);
int ccvpe_track_smooth(ccvpe_handle h, const float* belief, const float* smoothed_next, int32_t batch, const float* shift,
                       const float* taps, int32_t taps_stride, int32_t radius, const float* floor, float* smoothed,
                       float* stats, void* work, void* stream);
/* ccvpe_track_smooth for a stream tracked through ccvpe_track_predict_affine (KITTI's heading-up tiles): matrix, DEVICE float64
 * [batch][6], taps, taps_stride, radius, floor are the arguments of the ccvpe_track_predict_affine call that carried `belief` into
 * frame t + 1; every other argument is ccvpe_track_smooth's.  For a plane position y = (yx, yy) (integers, also outside the window)
 * take (sx, sy), ix, iy, fx, fy and det exactly as ccvpe_track_predict_affine computes them - the coordinates as float64 fma, floor,
 * the fraction rounded once to float32, det = (float)|m0 m4 - m1 m3| - and let wgt(y, x) be the float32 bilinear weight the sample
 * at y gives source cell x = (i, j): wx_a * wy_b with a = i - ix, b = j - iy both in {0, 1}, wx_0 = 1.f - fx, wx_1 = fx, likewise
 * along y; 0 when x is not one of the four cells.  Per query
 *     prior_i = Paff(belief; M)_i + floor              the bits ccvpe_track_predict_affine takes the logf of
 *     g_i     = s'_i > 0 ? s'_i / prior_i : 0
 *     G       = sum_i g_i
 *     h(y)    = (g, zero-extended, convolved with t[|k|] along x, then y)(y)   for y in [-radius, 511 + radius]^2, 0 beyond
 *     A(x)    = sum over y, rows ascending, then columns ascending, of det * (wy_b * (wx_a * h(y)))
 *               only terms with wx_a * wy_b > 0 enter the sum
 *     a_x     = fma(floor, G, A(x))
 *     w = belief * a,  Z = sum w,  smoothed = w * (1 / Z),  stats = (index, prob, Z, G)       as ccvpe_track_smooth
 * which inverts the transition T(x'|x) = det sum_y u(x' - y) wgt(y, x) + floor of that predict (u the separable tap kernel): the
 * blur is symmetric and moves to the g side, the adjoint of the resampling is taken on h.  That adjoint is a scatter; it is
 * computed as a gather - every cell walks the integer positions of the bounding box of the preimage of the open square
 * (i - 1, i + 1) x (j - 1, j + 1) under M and rejects those whose sample does not touch it - so nothing is accumulated
 * atomically and the same inputs give the same bits on every call, alone as in a batch.
 * Reach: with N the float64 inverse of [[m0, m1], [m3, m4]], hx = |N00| + |N01| and hy = |N10| + |N11|, a query is supported when
 * det is finite and non-zero and hx <= 3 and hy <= 3 (NaN fails): every rotation at scale >= 0.4715, every scale >= 0.5 at any
 * angle.  An unsupported link is a broken link: g = 0, so G = 0 and ccvpe_track_smooth's first rule holds - smoothed is belief
 * bit for bit, stats (argmax of belief, its value, NaN, 0).  det = 0 falls under this: that predict's prior is flat.  The other
 * degenerate rules, the independence of queries and the guards of every read are ccvpe_track_smooth's and
 * ccvpe_track_predict_affine's.  Relative error of smoothed against the exact recursion on the same float32 inputs and the same
 * float32 fractions: at most (16 radius + 141) * 2^-24 to first order - the count for ceil(2 hx) ceil(2 hy) <= 36 samples touching
 * one cell; DESIGN.md 4.22 has the table - when the coordinate arithmetic is exact in float64 (entries on a 2^-20 grid); otherwise
 * ccvpe_track_predict_affine's absolute term enters prior.
 * `work`: ccvpe_track_smooth_affine_work_bytes(batch) bytes (pure host arithmetic; 0 for batch <= 0), 16-byte aligned, any
 * contents: ccvpe_track_smooth's buffer, then h [576][576] per query.  Four launches, the last one ccvpe_track_smooth's.
 * CCVPE_EINVAL as ccvpe_track_smooth (a null matrix for a null shift). */
size_t ccvpe_track_smooth_affine_work_bytes(int32_t batch);
int ccvpe_track_smooth_affine(ccvpe_handle h, const float* belief, const float* smoothed_next, int32_t batch, const double* matrix,
                              const float* taps, int32_t taps_stride, int32_t radius, const float* floor, float* smoothed,
                              float* stats, void* work, void* stream);

/* Link statistics of a smoothed stream: what the stream itself says about the motion model of its tracker.  The transition of the
 * filter's hidden Markov model between frames t and t + 1 is T(x'|x) = u(x' - x - d) + floor; its pairwise posterior
 * p(x_t = x, x_t+1 = x' | frames 1..T) = b(x) T(x'|x) g(x') / Z, with g = s' / prior the ratio ccvpe_track_smooth forms, summed
 * over all pairs with one displacement x' - x, is the expected count of that transition - the E-step of Baum-Welch for `taps`,
 * `floor` and a bias of `shift`.  Arguments: ccvpe_track_smooth's - `belief` b, the filter posterior of frame t, `smoothed_next`
 * s', the smoothed map of frame t + 1, and shift, taps, taps_stride, radius, floor of the ccvpe_track_predict call that carried b
 * into frame t + 1.  Along each axis i = floor(d) clamped to +-2048 and f = d - floor(d), as that call splits a shift, and the
 * merged weights are u[k] = fmaf(f, t[|k - r|], (1.f - f) * t[|k - 1 - r|]), k = 0 .. 2r + 1 (t[j] = 0 for j > r); weight k
 * belongs to source column x' - ix - r - 1 + k of target column x'.  Per query, with K = 2 radius + 2,
 *     prior, g, G     exactly ccvpe_track_smooth's (the bits of its first launch)
 *     Sb              = sum_i b_i
 *     D[ky][kx]       = sum over the cells (y', x') of the window of
 *                       g(y', x') * b(y' - iy - r - 1 + ky, x' - ix - r - 1 + kx)             b zero-extended; ky, kx = 0 .. K - 1
 *     moves[ky][kx]   = fl(fl(uy[ky] * ux[kx]) * D[ky][kx])
 *     M = sum moves,  J = fl(fl(floor * G) * Sb),  Z = M + J
 * moves [batch][K][K] and stats [batch][4] = (Z, G, J, M), DEVICE float32, out.  moves[ky][kx] / Z is the posterior probability
 * that the link was a move under the motion kernel by the integer displacement x' - x = (ix + r + 1 - kx, iy + r + 1 - ky), J / Z
 * that it was a jump through the floor; Z is ccvpe_track_smooth's Z (sum s' over the taken cells) up to rounding.
 * There is no degenerate branch: every output is what the arithmetic gives.  A next map without a positive cell gives G = 0, zero
 * moves and Z = 0; a NaN in b gives that query NaN.  A link is usable when Z is finite and > 0.
 * Queries are independent: a poisoned query changes no bit of its neighbours.  No launch reads outside its tensors whatever the
 * inputs hold (ccvpe_track_predict's clamp and guards).  Every sum has a fixed order (kernels_track_link.hip lists them) and
 * nothing is accumulated atomically: the same inputs give the same bits on every call, alone as in a batch.
 * Relative error against the exact sums on the same float32 inputs, first order, every term non-negative, u = 2^-24: g
 * (4 radius + 14) u (ccvpe_track_smooth); a tile's D 37 u more (32 fused multiply-adds, 5 adds over the rows); an offset's 256 tile
 * sums 65 u; the two weights 2 u each, their product and the product with D 1 u each: moves (4 radius + 122) u.  M 26 u more (17 adds
 * in a thread, 6 over the wave, 3 over the waves): (4 radius + 148) u.  G (4 radius + 35) u and Sb 21 u (ccvpe_track_smooth's
 * orders), two products: J (4 radius + 58) u.  Z one add on the larger of the two: (4 radius + 149) u.
 * `work` is DEVICE memory of ccvpe_track_link_work_bytes(batch, radius) bytes (pure host arithmetic; 0 for batch <= 0 or radius
 * outside 0..32), 16-byte aligned, any contents: ccvpe_track_smooth's buffer for the batch, then 256 K K floats per query.  The
 * call allocates nothing, synchronises nothing and uses no scratch of the handle.  Four launches, the first one
 * ccvpe_track_smooth's.  CCVPE_EINVAL, nothing launched, checked before the handle is used: a null pointer, radius outside 0..32,
 * a taps_stride other than 0 or radius + 1, batch outside 1..4096, moves, stats or work equal to an input or to each other, a map
 * or work that is not 16-byte aligned.  smoothed_next == belief is allowed (nothing is written to a map). */
size_t ccvpe_track_link_work_bytes(int32_t batch, int32_t radius);
int ccvpe_track_link(ccvpe_handle h, const float* belief, const float* smoothed_next, int32_t batch, const float* shift,
                     const float* taps, int32_t taps_stride, int32_t radius, const float* floor, float* moves,
                     float* stats, void* work, void* stream);

/* The MAP trajectory of a tracked stream: the one most probable sequence of cells, which the argmaxes of T marginals are not.
 * The model is the filter's own mixture transition read as a latent choice per link: a link is a MOVE, with the merged kernel u
 * of ccvpe_track_predict, or a JUMP, with its floor; the path maximises over cells and link kinds jointly, which is
 * max(max_x u delta, floor max delta) and separable.  One call of ccvpe_track_viterbi per frame, from the first frame on, builds
 * the max-product score maps; one call of ccvpe_track_viterbi_back per link, from the last frame back, reads the path off them.
 * All maps DEVICE float32 [batch][512*512], n = 512*512: `belief` (b) the filter posterior of frame t (ccvpe_track_update's map),
 * `belief_prev` (b-) that of frame t - 1, `score_prev` (v-) the score map of frame t - 1 and `prev_stats` [batch][4] the stats of
 * the call that made it, `score` out.  shift (dx, dy), taps, taps_stride, radius, floor: the arguments of the ccvpe_track_predict
 * call that carried b- into frame t.  Along each axis, as that call splits a shift d: the integer part i = floor(d) clamped to
 * +-2048, the fraction f = d - floor(d), and the merged weights u[k] = fmaf(f, t[|k - r|], (1.f - f) * t[|k - 1 - r|]), k = 0 ..
 * 2r + 1 (a tap index above r reads 0); weight k belongs to source column x' - ix - r - 1 + k of target column x', likewise for
 * rows.  Per query, fl() one float32 rounding:
 *     prior_i = P(b-; dx, dy)_i + floor          the bits ccvpe_track_predict takes the logf of (ccvpe_track_smooth's prior)
 *     lik_i   = b_i > 0 ? b_i / prior_i : 0      the frame's likelihood up to a constant; NaN and negative b are not taken
 *     j       = (int) prev_stats[0] when 0 <= prev_stats[0] < n, else none;   peak = v-[j]
 *     win_i   = max over ky of fl(uy[ky] * max over kx of fl(ux[kx] * v-(source cell)))      v- zero-extended; each max taken
 *               as `c > acc ? c : acc` from acc = 0, so NaN and negatives never enter
 *     m_i     = max(win_i, fl(floor * peak))     move or jump (the jump enters when it is strictly larger)
 *     w_i     = fl(lik_i * m_i);  a w_i that is not > 0 (NaN included) counts and is stored as 0
 *     W       = max_i w_i at its first index i*;  e = the integer with W * 2^-e in [1, 2)
 *     score_i = ldexpf(w_i, -e)                  exact unless the result is subnormal
 *     stats   = (i*, score[i*], e, restarted)    float32 [4]
 *   - First frame: belief_prev, score_prev, prev_stats and shift all NULL.  w_i = b_i for b_i > 0, else 0; taps, taps_stride,
 *     radius and floor are not looked at and may be NULL or 0; restarted = 1.
 *   - Restart: j is none, or peak is not > 0 (the zero map behind a frame without a finite posterior).  m_i = 1, so w = lik, and
 *     restarted = 1; otherwise restarted = 0.
 *   - Degenerate: W is not > 0 or not finite.  An all-zero map and stats (-1, NaN, NaN, restarted).
 * The recursion has no sum of its own: the one blur is prior's, everything else is one float32 product and an exact maximum, and
 * the normalisation is by a power of two, so the frame-to-frame comparisons do not depend on it.  Relative error against a
 * float64 evaluation on the same float32 inputs, first order, u = 2^-24: lik (4 radius + 14) u, each merged weight 2 u, win 6 u,
 * the jump 1 u, w (4 radius + 21) u; the scaling adds none.  Queries are independent; no launch reads outside its tensors
 * whatever the inputs hold (ccvpe_track_predict's clamps and guards, and a guarded j); the same inputs give the same bits on
 * every call, alone as in a batch.  `work`: ccvpe_track_viterbi_work_bytes(batch) bytes of DEVICE memory (pure host arithmetic;
 * 0 for batch <= 0), 16-byte aligned, any contents: the 256 tile maxima per query between the two launches.  Two launches, in
 * the first-frame form as well.  The call allocates nothing, synchronises nothing and uses no scratch of the handle.
 * CCVPE_EINVAL, nothing launched, checked before the handle is used: a null belief, score, stats or work; a mix of NULL and
 * non-NULL among belief_prev, score_prev, prev_stats and shift; outside the first-frame form a null taps or floor, radius
 * outside 0..32, a taps_stride other than 0 or radius + 1; batch outside 1..4096; score or stats equal to an input, to work or
 * to each other (the step reads halos of its inputs: it cannot run in place); a map or work that is not 16-byte aligned.
 *
 * Backtrack of one link: `cell` DEVICE int32 [batch], the path's cell at frame t; back DEVICE int32 [batch][2] out =
 * (previous cell, kind), kind MOVE = 0, JUMP = 1, START = 2; score_prev, prev_stats and the predict arguments as above.
 *   - cell outside [0, n): (j or -1, START) - the end of a backtrack, or the frame behind a broken one.
 *   - otherwise j none: (-1, START).
 *   - otherwise the window candidates are the (2 radius + 2)^2 source cells of `cell` that lie inside the grid, each with the
 *     value fl(uy * fl(ux * v-)); the largest wins, the smallest source index on ties, NaN never; jump = fl(floor * v-[j]).
 *     Neither the best window value nor jump > 0: (j, START).  jump strictly larger than the best window value: (j, JUMP).
 *     Otherwise (best source cell, MOVE).
 * One launch, one workgroup per query, every read guarded.  CCVPE_EINVAL as above: a null pointer, the radius, taps_stride and
 * batch rules, back equal to an input, a score_prev that is not 16-byte aligned. */
size_t ccvpe_track_viterbi_work_bytes(int32_t batch);
int ccvpe_track_viterbi(ccvpe_handle h, const float* belief, const float* belief_prev, const float* score_prev,
                        const float* prev_stats, int32_t batch, const float* shift, const float* taps, int32_t taps_stride,
                        int32_t radius, const float* floor, float* score, float* stats, void* work, void* stream);
int ccvpe_track_viterbi_back(ccvpe_handle h, const float* score_prev, const float* prev_stats, const int32_t* cell, int32_t batch,
                             const float* shift, const float* taps, int32_t taps_stride, int32_t radius, const float* floor,
                             int32_t* back, void* stream);
/* The same two calls for a stream tracked through ccvpe_track_predict_affine (KITTI's heading-up tiles): matrix, DEVICE float64
 * [batch][6], taps, taps_stride, radius, floor are the arguments of the ccvpe_track_predict_affine call that carried b- into frame
 * t; b, b-, v-, prev_stats, j, peak and every other argument are ccvpe_track_viterbi's.  The maximum over the exact transition
 * T(x'|x) = det sum_y u(x' - y) wgt(y, x) + floor is not separable; the affine move is read as one more latent choice instead - of
 * the sample position y the blur reads, and of the one of that sample's four bilinear taps that carried the mass - as "move or
 * floor" already is.  For an integer plane position y (also outside the window) take (sx, sy), ix, iy, fx, fy and det exactly as
 * ccvpe_track_predict_affine computes them - the coordinates as float64 fma, then floor, the integer parts clamped to +-2048, the
 * fractions rounded once to float32, det = (float)|m0 m4 - m1 m3|; the four taps are (a, b) in {0, 1}^2 with source cell
 * (ix + a, iy + b) and weights wx_0 = 1.f - fx, wx_1 = fx, likewise along y; v- is zero-extended.  Per query, fl() one float32
 * rounding:
 *     prior_i = Paff(b-; M)_i + floor              the bits ccvpe_track_predict_affine takes the logf of
 *     lik_i   = b_i > 0 ? b_i / prior_i : 0
 *     cand(y, a, b) = fl(det * fl(wy_b * fl(wx_a * v-(ix + a, iy + b))))
 *     q(y)    = max over the four taps of cand     each max as `c > acc ? c : acc` from acc = 0
 *     win_i   = max over ky of fl(t[|ky - r|] * max over kx of fl(t[|kx - r|] * q(x' - r + kx, y' - r + ky))),   kx, ky = 0 .. 2r
 *     m_i     = max(win_i, fl(floor * peak))       the jump enters when it is strictly larger
 *     w, W, e, score, stats                        exactly ccvpe_track_viterbi's lines
 * The first-frame form (belief_prev, score_prev, prev_stats and matrix all NULL), the restart and the degenerate rules are
 * ccvpe_track_viterbi's, word for word; the first-frame form runs that call's two launches.  There is no reach rule: the recursion
 * only gathers.  det = 0, or a matrix that moves everything off the grid, gives win = 0, so every surviving link is a JUMP through
 * the floor; that follows from the definition and is no special case.  The matrix (1, 0, -dx, 0, 1, -dy) with integer dx, dy gives
 * ccvpe_track_viterbi's bits, score, stats and back.  The link weight of this model, T_aug(x'|x) = max over (y, tap) reaching x of
 * det u(x' - y) w_tap(y), satisfies T_aug <= T <= N T_aug with N = ceil(2 hx) ceil(2 hy) (hx, hy of ccvpe_track_smooth_affine: the
 * number of samples that can touch one cell), is positive wherever T is, and equals T at integer translations.
 * Backtrack of one link: the cell and j rules are ccvpe_track_viterbi_back's.  Otherwise the candidates are the 4 (2 radius + 1)^2
 * pairs of a sample position of the cell's window and one of its taps whose source cell lies inside the grid, each weighed
 * fl(t_y * fl(t_x * cand)); the largest wins, on ties the smallest source cell index, whatever sample it came through, NaN never;
 * jump and START / JUMP / MOVE as in ccvpe_track_viterbi_back.  Rounding is monotone and all factors are non-negative, so "max, then
 * multiply" in the step and "multiply, then max" in the backtrack pick the same value: a MOVE's candidate carries the bits of win.
 * Relative error against a float64 evaluation on the same float32 inputs, fractions and det, first order, u = 2^-24: lik
 * (4 radius + 14) u (ccvpe_track_predict_affine's (4 radius + 12) u on its sum, the floor add, the division), cand 5 u (1 - fx,
 * 1 - fy, three products), win 7 u, the jump 1 u, w (4 radius + 22) u; the scaling adds none.  Purely relative when the coordinate
 * arithmetic is exact in float64 (entries on a 2^-20 grid); otherwise ccvpe_track_predict_affine's absolute term enters prior.
 * Queries are independent; every read is guarded and clamped as in ccvpe_track_predict_affine; the same inputs give the same bits
 * on every call, alone as in a batch.  `work`: ccvpe_track_viterbi_work_bytes(batch) bytes.  Two launches per step, one per link;
 * nothing is allocated or synchronised, no scratch of the handle.  CCVPE_EINVAL as the two calls above, a null matrix standing where
 * a null shift stood. */
int ccvpe_track_viterbi_affine(ccvpe_handle h, const float* belief, const float* belief_prev, const float* score_prev,
                               const float* prev_stats, int32_t batch, const double* matrix, const float* taps,
                               int32_t taps_stride, int32_t radius, const float* floor, float* score, float* stats, void* work,
                               void* stream);
int ccvpe_track_viterbi_back_affine(ccvpe_handle h, const float* score_prev, const float* prev_stats, const int32_t* cell,
                                    int32_t batch, const double* matrix, const float* taps, int32_t taps_stride, int32_t radius,
                                    const float* floor, int32_t* back, void* stream);

/* Posterior summary: how sure the pose is. `summary` is float32 DEVICE memory [batch][16], one row per query, a function of the
 * float32 map h the same call would store as its posterior (h' of the definition above; log_prior NULL: ccvpe_forward's heatmap;
 * ccvpe_belief_summary: the map given), in cells of the 512 grid, x = index % 512 the column, y = index / 512 the row:
 *     0        argmax index as float: the first maximal index, NaN never wins, always a position inside the map
 *     1        h at the argmax                      (columns 0 and 1 carry the bits of rows[b][0..1])
 *     2        S0 = sum h                           (about 1 for a posterior; stored maps may be unnormalised)
 *     3        entropy -sum over h > 0 of (h / S0) ln(h / S0), nats
 *     4, 5     mean x, y = sum h x / S0, sum h y / S0
 *     6, 7, 8  var_xx, cov_xy, var_yy about that mean
 *     9        peak mass: sum h over the window |x - x*| <= radius, |y - y*| <= radius around the argmax (x*, y*), clipped to the
 *              grid, over S0
 *     10, 11   mean x, y of the window, weights h over the window's own sum
 *     12 - 14  var_xx, cov_xy, var_yy of the window about its own mean - the spread of the mode the argmax belongs to, without
 *              the distractors that inflate columns 6 - 8
 *     15       cells of the clipped window, as float
 * All sums are float64 (h times a coordinate product is exact there) in a fixed order: the same inputs give the same bits.
 * radius in 0..32.  A query without a finite posterior: rows (-1, NaN, ...) as ccvpe_localize_prior, summary (-1, NaN, NaN ...).
 * A stored map with S0 == 0: (0, 0, 0, NaN ...); one without a value above -inf (a belief is non-negative: outside the contract):
 * index 0, the map's value there, NaN moments - a position of the map whatever it holds.  rows [batch][5] are exactly the k == 0 rows of the matching prior form
 * (ccvpe_localize_prior, ccvpe_localize_prior_cached_indexed, ccvpe_postprocess_prior; log_prior NULL: ccvpe_track_update* without
 * a prior, i.e. ccvpe_localize*: logits without a finite (m', inv') - a NaN or +inf among them - give (-1, NaN) in every form).
 * log_prior may be NULL (prior_stride is then ignored); posterior may be NULL, else it receives ccvpe_track_update's map.  No
 * launch is added to the pose plans: the launch that finds the argmax reduces the sums, and its last workgroup recomputes the
 * window; ccvpe_belief_summary is one launch.  The pose forms run plans of their own (the float64 partial sums live in their
 * workspace) under the pose plans' launch names and tuning entries.  CCVPE_EINVAL, nothing launched, checked before the handle
 * is used: the null-pointer and batch checks of the matching prior form (log_prior and posterior excepted), a null summary,
 * radius outside 0..32, a bad prior_stride beside a prior, summary == rows, a posterior that is log_prior, logits, rows or
 * summary; ccvpe_belief_summary: a null or misaligned belief, a null summary, radius, batch outside 1..4096, summary == belief.
 * ccvpe_postprocess_summary and ccvpe_belief_summary: batch <= 4096, any handle, one call in flight per handle (they share the
 * scratch of ccvpe_postprocess_prior). */
int ccvpe_localize_summary(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const float* sat, int32_t batch,
                           const float* log_prior, int64_t prior_stride, int32_t radius, float* rows, float* summary,
                           float* posterior, void* stream);
int ccvpe_localize_summary_cached_indexed(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const void* cache,
                                          int32_t n_tiles, const int32_t* tile_index, int32_t batch, const float* log_prior,
                                          int64_t prior_stride, int32_t radius, float* rows, float* summary, float* posterior,
                                          void* stream);
int ccvpe_postprocess_summary(ccvpe_handle h, const float* logits, const float* ori, int32_t batch, const float* log_prior,
                              int64_t prior_stride, int32_t radius, float* rows, float* summary, float* posterior, void* stream);
/* The stored-map form: belief [batch][512*512] float32 DEVICE memory, 4-byte aligned (16-byte aligned maps are read faster) - a
 * full forward's heatmap, a tracker belief, any non-negative map. */
int ccvpe_belief_summary(ccvpe_handle h, const float* belief, int32_t batch, int32_t radius, float* summary, void* stream);

/* Heading posterior: the heading the network believes in, as a distribution.  Per query, over the n = 512 * 512 cells i of the
 * float32 map h the same call would store as its posterior (h' of the definition above) and the orientation field (c_i, s_i) =
 * ccvpe_forward's ori [batch][2][n]:
 *   - a cell is valid when c_i and s_i are finite and not both zero;
 *   - its angle a_i is the one rows[b][4] would carry for (c_i, s_i): acos(clamp(c, -1, 1)) in degrees, mirrored to (180, 360)
 *     for s < 0 - a float32 in [0, 360];
 *   - with nbins bins of width w = 360 / nbins, bin b covers [b w, (b + 1) w); a result >= nbins wraps to b - nbins, -0.0 is bin 0.
 *     Cells within about 1e-3 degree of an edge may land on either side of it.
 * `hist` is float32 DEVICE memory [batch][nbins]: hist[b] = sum of h_i over the valid cells of bin b - absolute mass, summed in
 * 2^-52 fixed point, so no result depends on the order of the additions.  `heading` is float32 DEVICE memory [batch][12]:
 *     0        M = sum of h_i over valid cells      (against the summary's S0: the mass without a heading)
 *     1, 2     C = sum h c / M, S = sum h s / M
 *     3        mean heading atan2(S, C) in degrees [0, 360), evaluated in float64; NaN when R == 0
 *     4        R = sqrt(C^2 + S^2), the mean resultant length; the circular variance is 1 - R
 *     5        mode bin as float: the first index of the maximal hist value; -1 for a query without a finite posterior
 *     6        hist[mode] / M
 *     7        M_w: M over the window |x - x*| <= radius, |y - y*| <= radius around the argmax, clipped to the grid - the
 *              window of the summary's columns 9 - 15
 *     8, 9     C_w, S_w over that window
 *     10, 11   mean heading and R of the window, by the rules of columns 3 and 4 - the heading of the mode the argmax belongs to
 * M, sum h c and sum h s are float64 sums in a fixed order: the same inputs give the same bits.  nbins in 4..360, radius in 0..32.
 * A query without a finite posterior: rows (-1, NaN, ...), heading NaN except column 5 = -1, hist all zero.  M == 0 with a
 * finite posterior (no valid cell): columns 0 and 7 are 0, the ratios NaN, the mode 0, hist all zero.  rows, summary and posterior
 * are ccvpe_localize_summary's for the same arguments; summary and posterior may be NULL, log_prior as well.  The pose forms run
 * plans of their own: the argmax pose plan with the whole orientation field computed into the workspace (the level-1 launch of
 * the full forward, under its name and tuning entry) and one more launch behind both decoders; the logits form is ccvpe_
 * postprocess_summary's launches plus that one.  CCVPE_EINVAL, nothing launched, checked before the handle is used: the checks of
 * the matching summary form (a null summary excepted), a null heading or hist, nbins outside 4..360, and heading or hist equal
 * to each other or to rows, log_prior, summary, posterior, logits or ori.  ccvpe_postprocess_heading shares the scratch of
 * ccvpe_postprocess_prior: batch <= 4096, one call in flight per handle. */
#define CCVPE_HEADING_COLS 12
#define CCVPE_HEADING_MAX_BINS 360
int ccvpe_localize_heading(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const float* sat, int32_t batch,
                           const float* log_prior, int64_t prior_stride, int32_t radius, int32_t nbins, float* rows, float* heading,
                           float* hist, float* summary, float* posterior, void* stream);
int ccvpe_localize_heading_cached_indexed(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const void* cache,
                                          int32_t n_tiles, const int32_t* tile_index, int32_t batch, const float* log_prior,
                                          int64_t prior_stride, int32_t radius, int32_t nbins, float* rows, float* heading,
                                          float* hist, float* summary, float* posterior, void* stream);
int ccvpe_postprocess_heading(ccvpe_handle h, const float* logits, const float* ori, int32_t batch, const float* log_prior,
                              int64_t prior_stride, int32_t radius, int32_t nbins, float* rows, float* heading, float* hist,
                              float* summary, float* posterior, void* stream);

/* Heading prior: information about the heading coming in - a compass reading, a gyro-propagated heading, the heading posterior of
 * the last frame.  The orientation field is the network's p(heading | position), so a prior over the heading is a per-cell
 * log-weight on the position grid.  The heading prior of a query is a table T of nb + 1 float32 log-weights in DEVICE memory, nb in
 * 4..360: entry b < nb belongs to heading bin b of the definition above ([b w, (b + 1) w), w = 360 / nb, the same angle and the
 * same binning code as hist), entry nb to a cell without a heading (an invalid cell of that definition).  Log-weights need not be
 * normalised; -inf excludes a bin.  table_stride is 0 (one table for every query) or nb + 1.  Per cell i of query b
 *     k_i = valid(c_i, s_i) ? bin_nb(c_i, s_i) : nb,     comb_i = T[k_i],  or  fl32(P_i + T[k_i]) with a position prior P
 * (one IEEE float add), and everything downstream is the position prior's definition with log_prior := comb, prior_stride :=
 * 512 * 512: l' = fl32(l + comb), the softmax statistics, the posterior h', and rows, summary, heading and hist of that posterior.
 * Every heading-prior form is bit-equal to the matching prior form fed the combined map; a query without a finite posterior - a
 * +inf or NaN in T on a bin some cell uses, every used entry -inf - gets the rows of that rule.  Cells within about 1e-3 degree of
 * a bin edge may take either neighbour's weight.  The approximation: the carried heading belief is treated as independent of the
 * position.
 *   ccvpe_heading_prior_map: one launch on forward outputs the caller holds (ori [batch][2][512*512]); out_map [batch][512*512]
 *     feeds any logits form (ccvpe_postprocess_prior, top-K included, _summary, _heading, ccvpe_track_update_logits) as its
 *     log_prior with stride 512 * 512.  log_prior may be NULL.  batch <= 4096, any handle, no scratch.
 *   ccvpe_localize_heading_prior, ccvpe_localize_heading_prior_cached_indexed: the outputs of ccvpe_localize_heading* of the
 *     posterior under both priors; nbins, the output histogram's bin count, is independent of nb.  tile_index may be NULL.  They
 *     run the heading plans with comb in the workspace and one launch more; the localisation tail then waits for the orientation
 *     decoder.  log_prior, summary and posterior may be NULL.
 *   ccvpe_heading_predict: the predict step on the heading axis, one launch.  hist [batch][nb] (non-negative: the hist of the
 *     last frame), turn_deg [batch] the heading change since that frame (positive: the heading angle grows), one-sided taps
 *     t[0..radius] (taps_stride 0 or radius + 1), floor [batch] >= 0, all DEVICE float32; out [batch][nb + 1], not aliasing hist.
 *     On the circle of nb bins: u = b - turn_deg / (360 / nb) in float64, i0 = floor(u), f = (float)(u - i0),
 *     s(b) = (1 - f) hist[i0 mod nb] + f hist[(i0 + 1) mod nb] (f == 0 weighs the one source bin with exactly 1), c = s circularly
 *     convolved with t[|j|], j = -radius..radius (2 radius + 1 fused multiply-adds), out[b] = logf(c(b) + floor) and
 *     out[nb] = logf((float)(float64 sum of c / nb) + floor): a cell without a heading weighs what the average bin does.  radius in
 *     0..32 with 2 radius + 1 <= nb.  An all-zero hist gives logf(floor) everywhere.  A non-finite turn_deg may give NaN, never a
 *     read outside hist.  batch 1..4096, any handle.
 * CCVPE_EINVAL, nothing launched, checked before the handle is used: a null pointer (log_prior, summary, posterior and tile_index
 * excepted), nb outside 4..360, table_stride other than 0 or nb + 1, radius outside its range or 2 radius + 1 > nb, a bad
 * taps_stride, the batch range, out_map equal to ori, log_prior or table, out == hist, a table that is an output, then the checks
 * of the matching heading form.  A debug handle gets CCVPE_ESTATE on the two network forms. */
int ccvpe_heading_prior_map(ccvpe_handle h, const float* ori, int32_t batch, const float* log_prior, int64_t prior_stride,
                            const float* table, int32_t table_stride, int32_t nb, float* out_map, void* stream);
int ccvpe_localize_heading_prior(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const float* sat, int32_t batch,
                                 const float* log_prior, int64_t prior_stride, const float* table, int32_t table_stride, int32_t nb,
                                 int32_t radius, int32_t nbins, float* rows, float* heading, float* hist, float* summary,
                                 float* posterior, void* stream);
int ccvpe_localize_heading_prior_cached_indexed(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const void* cache,
                                                int32_t n_tiles, const int32_t* tile_index, int32_t batch, const float* log_prior,
                                                int64_t prior_stride, const float* table, int32_t table_stride, int32_t nb,
                                                int32_t radius, int32_t nbins, float* rows, float* heading, float* hist,
                                                float* summary, float* posterior, void* stream);
int ccvpe_heading_predict(ccvpe_handle h, const float* hist, int32_t batch, int32_t nb, const float* turn_deg, const float* taps,
                          int32_t taps_stride, int32_t radius, const float* floor, float* out, void* stream);

/* Joint position-heading filter: a histogram filter over (heading bin k, cell i), which drops the approximation above.  The state
 * `joint` is float32 DEVICE memory [batch][nb][512*512]: one 512 x 512 map per heading bin in the pixel order of every other map,
 * bin k covering [k w, (k + 1) w) degrees, w = 360 / nb - hist's binning.  Values are linear (not logarithms) and non-negative.
 * nb in 4..72, batch >= 1, batch * nb <= 32768; every map pointer 16-byte aligned.  One step per frame =
 * ccvpe_track_joint_predict + ccvpe_track_joint_update_logits.
 *
 * Predict.  The motion model is x' = x + shift[heading], heading' = heading + turn, both halves blurred.  All pointers DEVICE:
 * shift [batch][nb][2] float32 = (dx, dy) in output pixels of every SOURCE heading bin (the kernel knows no angle convention: the
 * table carries it); taps, taps_stride, radius 0..32: the one-sided xy blur of ccvpe_track_predict; turn_deg [batch] (positive:
 * the heading angle grows); htaps the one-sided heading blur th[0..hradius], htaps_stride 0 or hradius + 1, hradius 0..32 with
 * 2 hradius + 1 <= nb; floor [batch] >= 0; work: ccvpe_track_joint_work_bytes(batch, nb) bytes, any contents; prior
 * [batch][nb][512*512] out, not aliasing joint or work.  Per query
 *     A(k', .)   = the map c of ccvpe_track_predict for the belief joint[k'], the shift shift[k'] and taps - the same arithmetic
 *     u          = k - turn_deg / w  (float64),  i0 = floor(u),  f = (float)(u - i0)
 *     g(k, i)    = (1 - f) A(i0 mod nb, i) + f A((i0 + 1) mod nb, i)         f == 0 weighs the one source bin with exactly 1
 *     C(k, i)    = sum over j = -hradius..hradius of th[|j|] g((k - j) mod nb, i)
 *     prior(k,i) = C(k, i) + floor
 * k is an integer, so i0 - k and f are those of k = 0 for every k, and the kernel takes them there: o = floor(-turn_deg / w),
 * f = (float)(-turn_deg / w - o).  The linear weights are folded into 2 hradius + 2 merged weights
 * M[d] = fmaf(f, th[|d - 1|], (1 - f) * th[|d|]), d = -hradius..hradius + 1 (th = 0 outside 0..hradius), and
 * C(k, i) = the fused multiply-adds M[d] * A((k + o + d) mod nb, i) in ascending d from a zero accumulator.  Every term is
 * non-negative, so the error is relative: prior is within (4 radius + 2 hradius + 18) * 2^-24 of the exact value on the same
 * float32 inputs - ccvpe_track_predict's (4 radius + 12), three roundings in a merged weight, 2 hradius + 2 fused multiply-adds
 * and the floor's add (first order; f as the kernel takes it).  Mass that leaves a map's window is lost; floor stands for it.
 * Non-finite shifts or turns may give NaN, but no launch reads outside its tensors whatever the inputs hold: the xy pass clamps and
 * guards as ccvpe_track_predict, the integer part of the turn is clamped to +-2^30 before it is converted and reduced modulo nb.
 * Two launches on the caller's stream; nothing of the handle but its device.
 *
 * Update, on ccvpe_forward's outputs logits [batch][512*512] and ori [batch][2][512*512], read as p(frame | position) and
 * p(heading | position).  prior [batch][nb][512*512] or NULL (the first frame: 1 everywhere).  emission: a table e of nb + 1
 * non-negative float32 weights, emission_stride 0 (one table) or nb + 1 (one per query): e[j], j < nb, weighs a heading j bins
 * ahead of the cell's own bin on the circle, e[nb] any heading at a cell without a valid orientation (valid and bin: the
 * definition of hist).  Per query
 *     m        = max l_i,  w_i = __expf(l_i - m)                            the statistics of the softmax above
 *     E(k | i) = valid(c_i, s_i) ? e[(k - bin_nb(c_i, s_i)) mod nb] : e[nb]
 *     U(k, i)  = (w_i * E(k | i)) * prior(k, i)                             float32 products, in this order
 *     Z        = sum over k, i of U                                         float64, fixed order
 *     J'(k, i) = U(k, i) * (float)(1 / Z)
 * joint_out [batch][nb][512*512] receives J'; it may be prior (in place).  marginal [batch][512*512] = the sum over k of J'(k, i)
 * in ascending k, float32: an ordinary belief map, to which ccvpe_belief_summary and ccvpe_belief_credible apply as they stand.
 * hist [batch][nb] = the sum over i of J'(k, i), a float64 sum in fixed order rounded once.  rows [batch][CCVPE_JOINT_COLS]:
 *   0 the first argmax cell of marginal, as float   1 marginal there   2 the first argmax bin of J'(., cell)   3 m   4 (float)Z
 * A query without a finite joint posterior - NaN or +inf in its logits, Z zero or not finite, or a positive Z so small (below
 * 2^-128) that (float)(1 / Z) is not finite - gets the row (-1, NaN, -1, m, Z)
 * and all-zero joint_out, marginal and hist, so that with a positive floor the next predict is flat and the stream starts over;
 * its batch neighbours keep their bits.  No float atomics: the same inputs give the same bits.  Four launches (the statistics,
 * the sum, the store, the finish); the joint moves through memory three times - prior read twice, J' written once.  The
 * handle's joint scratch grows with the largest batch seen; update calls on one handle run one at a time.  The predict's `work`
 * is the caller's: two predict calls in flight at once (two streams) need a work buffer each.
 * CCVPE_EINVAL, nothing launched, checked before the handle is used: a null pointer (prior of the update excepted), nb, radius,
 * hradius or the batch out of range, a bad taps_stride, htaps_stride or emission_stride, prior / joint / work of the predict
 * aliasing each other, an output of the update aliasing an input or another output (joint_out == prior excepted), a map
 * pointer that is not 16-byte aligned. */
#define CCVPE_JOINT_COLS 5
#define CCVPE_JOINT_MAX_BINS 72
size_t ccvpe_track_joint_work_bytes(int32_t batch, int32_t nb);
int ccvpe_track_joint_predict(ccvpe_handle h, const float* joint, int32_t batch, int32_t nb, const float* shift, const float* taps,
                              int32_t taps_stride, int32_t radius, const float* turn_deg, const float* htaps, int32_t htaps_stride,
                              int32_t hradius, const float* floor, void* work, float* prior, void* stream);
int ccvpe_track_joint_update_logits(ccvpe_handle h, const float* logits, const float* ori, int32_t batch, const float* prior,
                                    const float* emission, int32_t emission_stride, int32_t nb, float* rows, float* joint_out,
                                    float* marginal, float* hist, void* stream);

/* The joint predict across frames whose grids differ by more than a translation (KITTI's heading-up tiles): every SOURCE heading bin
 * is carried through an affine map of its own.  matrix is float64 DEVICE memory [batch][nb][6]: matrix[b][k'] maps an OUTPUT pixel
 * index to the SOURCE index position that bin k' reads, in the convention of ccvpe_track_predict_affine.  In the intended use the
 * matrices of a query share their linear part - the frame change - and differ in the translation column alone - the motion as each
 * heading sees it; nothing here assumes that.  Every other argument, with its range, is ccvpe_track_joint_predict's; work is
 * ccvpe_track_joint_work_bytes(batch, nb) bytes; prior aliases neither joint nor work.  Per query
 *     A(k', .)   = the map c of ccvpe_track_predict_affine for the belief joint[k'], the matrix matrix[k'] and taps
 *                  (|det| included, the same arithmetic, before floor and log)
 *     prior(k,i) = ccvpe_track_joint_predict's C(k, i) + floor over these A: o, f, M[d], the fmaf chain in ascending d, unchanged
 * so the matrices (1, 0, -dx[k'], 0, 1, -dy[k']) with integer shifts give ccvpe_track_joint_predict's bits, and one matrix for every
 * bin with hradius 0, turn 0 and htaps (1) gives exp of ccvpe_track_predict_affine's map, slice by slice.  Every term is
 * non-negative: prior is within (4 radius + 2 hradius + 18) * 2^-24 of the exact value on the same float32 inputs, plus
 * ccvpe_track_predict_affine's coordinate term 2^-38 max(joint of the query).  No matrix, NaN included, moves a read outside joint:
 * the integer parts are clamped before they are converted and every read is bounds-checked; the turn is clamped as above.  A
 * singular matrix gives A = 0 for its bin.  Two launches on the caller's stream - the affine sampling and the xy blur of every
 * slice, grid (256 tiles, batch * nb), then ccvpe_track_joint_predict's heading mix -, no atomics: the same inputs give the same
 * bits, alone as in a batch.  CCVPE_EINVAL as ccvpe_track_joint_predict, in its order, `matrix` in the place of `shift`. */
int ccvpe_track_joint_predict_affine(ccvpe_handle h, const float* joint, int32_t batch, int32_t nb, const double* matrix,
                                     const float* taps, int32_t taps_stride, int32_t radius, const float* turn_deg,
                                     const float* htaps, int32_t htaps_stride, int32_t hradius, const float* floor,
                                     void* work, float* prior, void* stream);

/* Smoothing a joint stream: the backward half of the joint filter.  One call per frame, from the last frame back, turns the stored
 * joints into p(cell, heading bin | frames 1..T).  `joint` J is the stored filter joint of frame t (ccvpe_track_joint_update_logits'
 * joint_out), `smoothed_next` s' the smoothed joint of frame t + 1 (for the last frame but one: the last frame's own J), both DEVICE
 * float32 [batch][nb][512*512]; shift, taps, taps_stride, radius, turn_deg, htaps, htaps_stride, hradius, floor: the arguments of the
 * ccvpe_track_joint_predict call that carried J into frame t + 1, with its ranges.  With P(m; d), o, f and M[d] as above, per query
 *     A(k')      = P(J[k']; shift[k'])                                   the predict's first launch, unchanged
 *     prior(k,i) = (fmaf chain of M[d] A((k + o + d) mod nb, i), ascending d) + floor     the bits the predict stores
 *     g(k,i)     = s'(k,i) > 0 ? s'(k,i) / prior(k,i) : 0                NaN and negative s' are not taken
 *     G          = sum over k, i of g                                    float64, one fixed order
 *     h(k',i)    = sum over d = -hradius..hradius+1, ascending, of fmaf(M[d], g((k' - o - d) mod nb, i), h)
 *     a(k',i)    = fmaf(floor, (float)G, P(h[k']; -shift[k'])_i)
 *     w(k',i)    = J(k',i) * a(k',i);   Z = float64 sum of w, fixed order
 *     s(k',i)    = w(k',i) * (float)(1 / Z)
 * For a J of mass 1 the predict is prior = T J with T((k,x) | (k',x')) = sum over d with (k + o + d) mod nb == k' of
 * M[d] u_k'(x - x' - shift[k']) + floor, and the recursion is s = J . (T^t g), g = s' / prior.  The adjoint of the circle mix sends
 * g(k) to every k' = (k + o + d) mod nb with weight M[d] - the line for h, which runs the other way round the circle and covers
 * 2 hradius + 2 > nb, where two d meet in one bin; the adjoint of P(.; shift[k']) is P(.; -shift[k']) (taps and tent are even) with
 * each SOURCE bin's own shift; the floor's is floor * G.  Z = sum g prior = sum s' over the taken cells: 1 up to rounding.
 * Outputs: smoothed [batch][nb][512*512] = s; marginal [batch][512*512] = the sum over k of s(k, i), ascending k, float32; hist
 * [batch][nb] = the float64 sum over i of s(k, i), rounded once; stats [batch][CCVPE_JOINT_SMOOTH_COLS] = (index, prob, bin,
 * (float)Z, (float)G): index the first argmax cell of marginal, prob marginal there (its stored bits), bin the first argmax of
 * s(., index).
 *   - G == 0 (s' has no positive value - the zero joint of a frame without a finite posterior, the call for the last frame): the
 *     future says nothing; s is J bit for bit, marginal, hist, index, prob, bin are those of J (a value is taken when it is above
 *     -inf, NaN never wins, the first index wins ties; no taken value: -1, NaN, -1), Z = NaN, G = 0.
 *   - else Z not finite, Z <= 0, or positive but without a finite (float)(1 / Z) (a zero J, a NaN in J, floor = 0 and a prior of 0
 *     under a positive s'): zeros everywhere and (-1, NaN, -1, Z, G).
 * Queries are independent: a poisoned query changes no bit of its neighbours.  No input value moves a read outside a tensor (the
 * predict's clamps of the shift and of the turn's integer part).  Every sum has a fixed order and nothing is accumulated atomically:
 * the same inputs give the same bits, alone as in a batch.  Relative error of smoothed against the exact recursion on the same
 * float32 inputs: (16 radius + 8 hradius + 78) * 2^-24 to first order, marginal nb more, hist 1 more.
 * `work`: DEVICE memory of ccvpe_track_joint_smooth_work_bytes(batch, nb) bytes (pure host arithmetic; 0 outside the ranges), 16-byte
 * aligned, any contents: one joint-sized buffer (A, then h) and the partial sums; nothing in it has to survive a call.  The call
 * allocates nothing, synchronises nothing and uses no scratch of the handle: calls on several streams of one handle may run at once
 * when each has its own work and outputs.  `smoothed` may be `smoothed_next`: a backward sweep runs in one buffer, with the bits of
 * the out-of-place call.  Five launches; the joint moves through memory ten times (2 + 3 + 3 + 2).  CCVPE_EINVAL, nothing launched,
 * checked before the handle is used: a null pointer, nb, radius, hradius or the batch out of range, a bad taps_stride or
 * htaps_stride, an output equal to an input, to work or to another output (smoothed == smoothed_next excepted), joint, smoothed_next
 * and work equal to each other, a map or work that is not 16-byte aligned. */
#define CCVPE_JOINT_SMOOTH_COLS 5
size_t ccvpe_track_joint_smooth_work_bytes(int32_t batch, int32_t nb);
int ccvpe_track_joint_smooth(ccvpe_handle h, const float* joint, const float* smoothed_next, int32_t batch, int32_t nb, const float* shift,
                             const float* taps, int32_t taps_stride, int32_t radius, const float* turn_deg, const float* htaps,
                             int32_t htaps_stride, int32_t hradius, const float* floor, void* work, float* smoothed, float* marginal,
                             float* hist, float* stats, void* stream);

/* The MAP trajectory of a joint stream: the one most probable sequence of (cell, heading bin) - a full (x, y, heading) track, which
 * neither the argmaxes of T smoothed marginals nor "the best bin there" are.  The model is the joint filter's own transition read as
 * a latent choice per link: the source bin offset d (which of the 2 hradius + 2 merged circle weights M[d] carried the mass), the
 * window position under the source bin's shift (as in ccvpe_track_viterbi), or a JUMP through the floor to any state.  One call of
 * ccvpe_track_joint_viterbi per frame, from the first frame on, builds the score joints; one call of
 * ccvpe_track_joint_viterbi_back per link, from the last frame back, reads the path off them.  All joints DEVICE float32
 * [batch][nb][512*512], n = 512*512: `joint` (J) the filter joint of frame t (ccvpe_track_joint_update_logits' joint_out),
 * `joint_prev` (J-) that of frame t - 1, `score_prev` (v-) the score joint of frame t - 1 and `prev_stats`
 * [batch][CCVPE_JOINT_VITERBI_COLS] the stats of the call that made it, `score` out.  shift [batch][nb][2], taps, taps_stride,
 * radius, turn_deg, htaps, htaps_stride, hradius, floor: the arguments of the ccvpe_track_joint_predict call that carried J- into
 * frame t, with its ranges.  With P(m; d), o, f and M[d] as in that call and ux, uy the merged weights of ccvpe_track_viterbi under
 * shift[k'], per query, fl() one float32 rounding:
 *     A(k')      = P(J-[k']; shift[k'])                                  the predict's first launch, unchanged
 *     prior(k,i) = (fmaf chain of M[d] A((k + o + d) mod nb, i), ascending d) + floor     the bits the predict stores
 *     lik(k,i)   = J(k,i) > 0 ? J(k,i) / prior(k,i) : 0                  NaN and negative J are not taken
 *     (jk, j)    = ((int) prev_stats[1], (int) prev_stats[0]) when 0 <= prev_stats[0] < n and 0 <= prev_stats[1] < nb, else none
 *     win(k',i)  = max over ky of fl(uy[ky] * max over kx of fl(ux[kx] * v-(k', source cell)))      per SOURCE bin, under shift[k']
 *     mix(k,i)   = max over d = -hradius..hradius+1 of fl(M[d] * win((k + o + d) mod nb, i))
 *     m(k,i)     = max(mix(k,i), fl(floor * v-(jk, j)))                  move or jump (the jump enters when it is strictly larger)
 *     w(k,i)     = fl(lik * m);  a w that is not > 0 (NaN included) counts and is stored as 0
 *     W          = max over (k, i) of w at its first flat index k n + i;  e = the integer with W * 2^-e in [1, 2): one per query
 *     score      = ldexpf(w, -e)                                         exact unless the result is subnormal
 *     stats      = (i*, k*, score(k*, i*), e, restarted)                 float32 [5]: cell and bin are separate columns, the flat
 *                                                                        index reaches 18.9 M at nb 72 and float32 cannot hold that
 * Every maximum takes its candidates as `c > acc ? c : acc` from acc = 0, so NaN and negatives never enter.  When 2 hradius + 1 == nb
 * two offsets d reach one source bin with different weights; the maximum takes the larger.
 *   - First frame: joint_prev, score_prev, prev_stats and shift all NULL.  w = J for J > 0, else 0; the other motion arguments are
 *     not looked at and may be NULL or 0; restarted = 1.
 *   - Restart: (jk, j) is none, or v-(jk, j) is not > 0 (the zero joint behind a frame without a finite posterior).  m = 1, so
 *     w = lik, and restarted = 1; otherwise restarted = 0.
 *   - Degenerate: W is not > 0 or not finite.  An all-zero score joint and stats (-1, -1, NaN, NaN, restarted).
 * The recursion has no sum of its own beyond the prior's, and the normalisation is by a power of two.  Relative error against a
 * float64 evaluation on the same float32 inputs, first order, u = 2^-24: the prior (4 radius + 2 hradius + 18) u, lik one more, a
 * window candidate 6 u, M[d] 3 u, a mix candidate 10 u, the jump 1 u, w (4 radius + 2 hradius + 30) u; the scaling adds none
 * (DESIGN.md 4.29).  Queries are independent: a query under any of the rules leaves its neighbours' bits unchanged; no launch reads
 * outside its tensors whatever the inputs hold (the predict's clamps of the shifts and of the turn's integer part, and a guarded
 * (jk, j)); the same inputs give the same bits on every call, alone as in a batch.  `work`:
 * ccvpe_track_joint_viterbi_work_bytes(batch, nb) bytes of DEVICE memory (pure host arithmetic; 0 outside the ranges), 16-byte
 * aligned, any contents: two joint-sized buffers (A and win) and the 1024 group maxima per query.  Four launches per step - the
 * predict's first launch on J-, the window maxima, the mix, the scale - and two, the last two, in the first-frame form; the joint
 * moves through memory ten times (2 + 2 + 4 + 2).  The call allocates nothing, synchronises nothing and uses no scratch of the
 * handle.  CCVPE_EINVAL, nothing launched, checked before the handle is used: a null joint, work, score or stats; a mix of NULL and
 * non-NULL among joint_prev, score_prev, prev_stats and shift; outside the first-frame form a null taps, turn_deg, htaps or floor,
 * radius or hradius out of range, a bad taps_stride or htaps_stride; nb outside 4..72, batch * nb above 32768; score or stats
 * equal to an input, to work or to each other (the step reads halos of its inputs: it cannot run in place); a joint or work that
 * is not 16-byte aligned.
 *
 * Backtrack of one link: `cell`, `bin` DEVICE int32 [batch], the path's pair at frame t; back DEVICE int32 [batch][3] out =
 * (previous cell, previous bin, kind), kind MOVE = 0, JUMP = 1, START = 2; the other arguments as above.
 *   - cell outside [0, n) or bin outside [0, nb): (j, jk, START), or (-1, -1, START) where (jk, j) is none - the end of a
 *     backtrack, or the frame behind a broken one.
 *   - otherwise (jk, j) none: (-1, -1, START).
 *   - otherwise the candidates are fl(M[d] * fl(uy * fl(ux * v-(k', g)))) over d and the (2 radius + 2)^2 source cells g of `cell`
 *     in the window of k' = (bin + o + d) mod nb under shift[k'] that lie inside the grid; the largest wins, the smallest flat source
 *     index k' n + g on ties, NaN never; jump = fl(floor * v-(jk, j)).  Neither the best candidate nor jump > 0: (j, jk, START).
 *     jump strictly larger than the best candidate: (j, jk, JUMP).  Otherwise (g, k', MOVE) of the best candidate.
 * Rounding is monotone and all factors are non-negative, so the best candidate's value is mix(bin, cell) bit for bit.  One launch,
 * one workgroup per query, every read guarded.  CCVPE_EINVAL as above: a null pointer, the range and stride rules, back equal to
 * an input, a score_prev that is not 16-byte aligned. */
#define CCVPE_JOINT_VITERBI_COLS 5
size_t ccvpe_track_joint_viterbi_work_bytes(int32_t batch, int32_t nb);
int ccvpe_track_joint_viterbi(ccvpe_handle h, const float* joint, const float* joint_prev, const float* score_prev,
                              const float* prev_stats, int32_t batch, int32_t nb, const float* shift, const float* taps,
                              int32_t taps_stride, int32_t radius, const float* turn_deg, const float* htaps, int32_t htaps_stride,
                              int32_t hradius, const float* floor, void* work, float* score, float* stats, void* stream);
int ccvpe_track_joint_viterbi_back(ccvpe_handle h, const float* score_prev, const float* prev_stats, const int32_t* cell,
                                   const int32_t* bin, int32_t batch, int32_t nb, const float* shift, const float* taps,
                                   int32_t taps_stride, int32_t radius, const float* turn_deg, const float* htaps,
                                   int32_t htaps_stride, int32_t hradius, const float* floor, int32_t* back, void* stream);

/* Credible regions: the smallest set of cells holding a share of the posterior (the highest-density region of a histogram
 * posterior).  Per query, over the n = 512 * 512 cells of a float32 map h - ccvpe_belief_credible: the map given; the other forms:
 * the posterior h' of the prior forms, the map ccvpe_track_update* stores (all zero for a query without a finite posterior):
 *   key    k_i = the uint32 bit pattern of h_i when h_i > 0, else 0.  +inf is a value; NaN, zero and negative values have key 0.
 *          Positive floats order as their bit patterns do.
 *   mass   q_i = (uint64) floorf(fminf(h_i, 1.f) * 2^44) when h_i > 0, else 0: an exact scaling and one truncation.  A value above
 *          1 is outside the contract: it is ordered by its value and weighs 1.  A cell below 2^-44 has a key and no mass.
 *   total  Q = sum q_i, an exact uint64 (n * 2^44 = 2^62).  G(k) = sum of q_i over k_i >= k, C(k) = count of k_i >= k.
 *   level  p, a float32 in (0, 1]: T = (uint64) ceil((double)p * (double)Q), raised to 1 and capped at Q.  k* = the largest key
 *          present in the map with G(k*) >= T; the region is { i : k_i >= k* } - closed under ties, the smallest union of whole
 *          value classes that holds at least the share p.  It exists whenever Q > 0.
 *   probe  optional, one cell index per query (DEVICE int32 [batch], NULL: none): above = sum of q_i over k_i > k_probe,
 *          rank = count of k_i > k_probe.  The cell lies in the region of level p exactly when above < T(p).  An index outside
 *          [0, n) gives NaN for both and nothing is read there (the rule of gt_index in ccvpe_eval_metrics).
 * `cred` is float32 DEVICE memory [batch][4 + 3 * n_levels]:
 *     0        (float)((double)Q * 2^-44)
 *     1        cells with h > 0
 *     2        probe: (float)((double)above / (double)Q); NaN without a probe, with a bad index, or when Q == 0
 *     3        probe: rank; NaN without a probe or with a bad index
 *     4 + 3j   level j: the threshold value, the float whose bits are k*
 *     5 + 3j   level j: C(k*), the region's area in cells (exact, at most 2^18)
 *     6 + 3j   level j: (float)((double)G(k*) / (double)Q), at least p up to that one rounding
 * Q == 0: the level columns are (NaN, 0, NaN).  `level_map` (optional, NULL: none) is uint8 DEVICE memory [batch][n]: cell i holds
 * the number of requested levels whose region contains it - with ascending levels a contour map, a value >= n_levels - j marks
 * the region of level j; all zero when Q == 0.  `levels` is HOST float32 [n_levels], 1 <= n_levels <= 8, each finite and in
 * (0, 1], any order, repeats allowed; they travel in the launch arguments (no copy to the device, no synchronisation, the array
 * may be reused when the call returns).  Every number is an integer or one correctly rounded float64 operation on integers: the
 * same inputs give the same bits in every form, on every run.
 *   ccvpe_belief_credible: a stored map (4-byte aligned; 16-byte aligned maps are read as float4).  4 launches, 5 with a
 *     level_map, per 256 queries of the batch.
 *   ccvpe_postprocess_credible: rows and the optional posterior of ccvpe_track_update_logits, cred and level_map of
 *     ccvpe_belief_credible on that posterior, bit for bit, whether or not it is stored.  The launches of
 *     ccvpe_track_update_logits plus those of ccvpe_belief_credible.
 *   ccvpe_localize_credible, ccvpe_localize_credible_cached_indexed (tile_index may be NULL): the same for
 *     ccvpe_track_update / ccvpe_track_update_cached_indexed; plans of their own, the argmax pose plan with the credible launches
 *     (4, 5 with a level_map) behind pose.argmax.
 * log_prior, probe, level_map and posterior may be NULL.  CCVPE_EINVAL, nothing launched, checked before the handle is used: a
 * null pointer other than those, n_levels outside 1..8, a level that is not finite or not in (0, 1], a bad prior_stride beside a
 * prior, batch outside 1..4096 (stored-map and logits forms), a misaligned belief, cred or level_map equal to each other or to
 * any input or other output; then the checks of the matching ccvpe_track_update form.  CCVPE_ESTATE on a debug handle for the two
 * network forms.  The stored-map and logits forms share the scratch of ccvpe_postprocess_prior: one call in flight per handle. */
#define CCVPE_CREDIBLE_MAX_LEVELS 8
int ccvpe_belief_credible(ccvpe_handle h, const float* belief, int32_t batch, const float* levels, int32_t n_levels,
                          const int32_t* probe, float* cred, uint8_t* level_map, void* stream);
int ccvpe_postprocess_credible(ccvpe_handle h, const float* logits, const float* ori, int32_t batch, const float* log_prior,
                               int64_t prior_stride, const float* levels, int32_t n_levels, const int32_t* probe, float* rows,
                               float* cred, uint8_t* level_map, float* posterior, void* stream);
int ccvpe_localize_credible(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const float* sat, int32_t batch,
                            const float* log_prior, int64_t prior_stride, const float* levels, int32_t n_levels,
                            const int32_t* probe, float* rows, float* cred, uint8_t* level_map, float* posterior, void* stream);
int ccvpe_localize_credible_cached_indexed(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const void* cache,
                                           int32_t n_tiles, const int32_t* tile_index, int32_t batch, const float* log_prior,
                                           int64_t prior_stride, const float* levels, int32_t n_levels, const int32_t* probe,
                                           float* rows, float* cred, uint8_t* level_map, float* posterior, void* stream);

/* Input pre-processing on device (reference train_VIGOR.py:57-70 ToTensor + Normalize, datasets.py:118
 * torch.roll(grd, shift, dims=2), train_VIGOR.py:272-273 FoV crop): uint8 HWC images [B,H,W,3] (decoded and
 * resized on the host) -> float32 NCHW [B,3,H,crop_w] with out[..., x] = norm(in[..., (x - shift[b]) mod W, :]).
 * `shift` is DEVICE memory [B] or NULL; mean/std are host arrays of 3.  Bit-identical to torchvision's fp32
 * (x/255 - mean)/std. */
int ccvpe_preprocess(const uint8_t* hwc, int32_t batch, int32_t H, int32_t W, const int32_t* shift, int32_t crop_w,
                     const float mean[3], const float stdv[3], float* out_nchw, void* stream);

/* The same with the resize in front (reference train_VIGOR.py:57-70 transforms.Resize([320,640]) / Resize([512,512]), applied
 * to PIL images at datasets.py:106, i.e. PIL.Image.resize(BILINEAR)): uint8 HWC images [B,in_h,in_w,3] as decoded ->
 * Pillow's 8-bit bilinear resampler (triangle filter with support = the down-scaling factor, 22-bit fixed-point taps,
 * horizontal pass first, uint8 between the passes; byte-identical to PIL) -> ToTensor + Normalize + roll + crop as above ->
 * float32 NCHW [B,3,out_h,crop_w].  `scratch` is caller-owned DEVICE memory of batch*in_h*out_w*3 bytes (may be NULL when
 * in_w == out_w).  Down-scaling factors above 8 per axis are refused. */
int ccvpe_preprocess_resize(const uint8_t* hwc, int32_t batch, int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w,
                            const int32_t* shift, int32_t crop_w, const float mean[3], const float stdv[3], uint8_t* scratch,
                            float* out_nchw, void* stream);

/* Aerial preparation of the KITTI test loop on device (reference datasets.py:577-598 SatGrdDatasetTest: sat_map.rotate(-heading),
 * transform(AFFINE, camera-GPS shift, BILINEAR), transform(AFFINE, test-split shift, BILINEAR), rotate(theta * rotation_range),
 * TF.center_crop(512), then satmap_transform = Resize (a copy at 512^2) + ToTensor + Normalize, train_KITTI.py:60-64).
 * uint8 HWC tiles [B,H,W,3] -> a chain of n_stages PIL affine resamplings, each output pixel (x, y) of a stage taking the
 * input position (m0*x' + m1*y' + m2, m3*x' + m4*y' + m5) of PIL's `data` tuple (x' = x + 0.5 for BILINEAR, Pillow's own
 * pixel-centre conventions for each filter), every stage an H x W canvas with 0 outside, uint8 between stages, byte-identical
 * to Pillow -> the out_h x out_w window at (top, left) of the last canvas -> ToTensor + Normalize -> float32 NCHW
 * [B,3,out_h,out_w].  `matrices` is DEVICE memory [B][n_stages][6] (double, stage 0 reads the input); `filters` is a host
 * array [n_stages] of CCVPE_RESAMPLE_NEAREST / CCVPE_RESAMPLE_BILINEAR (PIL.Image.NEAREST / BILINEAR); mean/std as above.
 * NEAREST stages are Pillow's 16.16 fixed-point path, which Pillow takes while the canvas corners map inside +-32768:
 * every rotation about the centre (Image.rotate, including its copy / transpose shortcuts) qualifies.  CCVPE_EINVAL, with
 * nothing launched: a null pointer, n_stages outside 1..4, more than 2 BILINEAR stages, an unknown filter, a side above
 * 16384, batch above 65535, a crop window outside the canvas. */
#define CCVPE_RESAMPLE_NEAREST 0
#define CCVPE_RESAMPLE_BILINEAR 2
int ccvpe_preprocess_affine(const uint8_t* hwc, int32_t batch, int32_t H, int32_t W, const double* matrices, const int32_t* filters,
                            int32_t n_stages, int32_t top, int32_t left, int32_t out_h, int32_t out_w, const float mean[3],
                            const float stdv[3], float* out_nchw, void* stream);

/* Aerial preparation of the Oxford test loop on device (reference datasets.py:306-321: full_satellite_map.crop((x0, y0,
 * x0 + win_w, y0 + win_h)) on the 400-px grid, then transform_sat = Resize([512,512]) + ToTensor + Normalize,
 * train_OxfordRobotCar.py:56-60): ONE resident uint8 map [map_h,map_w,3] (DEVICE) -> per sample the win_h x win_w window whose
 * top-left corner is origins[b] = (x0, y0) (DEVICE int32 [B][2], PIL's crop-box order; pixels outside the map are 0, as
 * PIL's crop fills them) -> the same Pillow-exact bilinear resize as ccvpe_preprocess_resize to out_h x out_w -> ToTensor +
 * Normalize -> float32 NCHW [B,3,out_h,out_w].  `scratch` is caller-owned DEVICE memory of batch*win_h*out_w*3 bytes, always
 * required.  CCVPE_EINVAL: a null pointer, a non-positive size, a down-scaling factor above 8. */
int ccvpe_preprocess_window_resize(const uint8_t* map_hwc, int32_t map_h, int32_t map_w, const int32_t* origins, int32_t batch,
                                   int32_t win_h, int32_t win_w, int32_t out_h, int32_t out_w, const float mean[3], const float stdv[3],
                                   uint8_t* scratch, float* out_nchw, void* stream);

/* Debug taps: when enabled, intermediate tensors of the next forward call stay resident and can be
 * copied out by name as NCHW float32 into HOST memory (`capacity` in floats).  Returns the number
 * of floats written via *n_out.  Names: see DESIGN.md (e.g. "sat_block15", "loc_level6"). */
int ccvpe_set_debug(ccvpe_handle h, int32_t enable);
/* Issue order of the next forward calls: 2 (default) = the aerial encoder and the orientation decoder run on an internal
 * second stream; 1 = everything in program order on the caller's stream.  Results are bit-identical (test hook and
 * diagnostic switch; no reference counterpart). */
int ccvpe_set_streams(ccvpe_handle h, int32_t n_streams);
int ccvpe_read_tap(ccvpe_handle h, const char* name, float* host_dst, size_t capacity, size_t* n_out,
                   int32_t shape_out[4]);

/* Diagnostic: after a synchronised forward, writes one text line per launch of its plan (name, stream, cross-stream
 * wait, tile) with an integer checksum of every tensor the launch touches.  Meaningful for plans whose tensors keep
 * their memory (debug plans, two-stream plans issued either way): diffing two dumps names the first launch whose
 * output differs.  No reference counterpart. */
int ccvpe_debug_dump_plan(ccvpe_handle h, const char* path);

/* Per-kernel device timing of the most recent ccvpe_profile_forward call: runs one forward with a
 * hipEvent pair around every launch and reports (name, milliseconds) rows.  Used by bench.py for
 * the roofline line.  Returns the number of rows; row i is copied into name_buf / ms. */
int ccvpe_profile_forward(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const float* sat,
                          int32_t batch, const ccvpe_outputs* out, void* stream);
int ccvpe_profile_row(ccvpe_handle h, int32_t i, char* name_buf, size_t name_cap, float* ms,
                      double* flops, double* bytes);
/* FLOPs row i actually issued on the matrix pipe: M / N padded to the launch's tile, K to the packed depth, 16
 * products per 2x2 tile for the Winograd tiles, three MFMAs per product in bf16x3 mode (`flops` of
 * ccvpe_profile_row is the algorithmic direct-convolution count). */
int ccvpe_profile_row_issued(ccvpe_handle h, int32_t i, double* issued_flops);

/* Kernel-level hook for parity tests and tile tuning (not on the product path): one NHWC fp32
 * convolution through the implicit-GEMM MFMA kernel.  in [B,H,W,Cin] (device, Cin % 8 == 0),
 * w [Cout,Cin,KH,KW] and bias [Cout] in the reference's layout (host or device; bias may be NULL),
 * symmetric zero padding `pad`, out [B,OH,OW,Cout] (device) with OH = (H + 2*pad - KH)/stride + 1.
 * act: 0 none, 1 relu, 2 swish.  tile: 0 = heuristic, else an internal tile id (1..ccvpe_op_num_tiles()).
 * iters > 0 additionally times `iters` back-to-back launches with hipEvents and stores the mean
 * milliseconds in *ms. */
int ccvpe_op_num_tiles(void);
const char* ccvpe_op_tile_name(int32_t tile);   /* tile ids are 1..ccvpe_op_num_tiles() */
int ccvpe_op_conv2d(const float* in, int32_t B, int32_t H, int32_t W, int32_t Cin, const float* w, const float* bias,
                    int32_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t pad, int32_t act, int32_t tile,
                    float* out, int32_t iters, float* ms, void* stream);

/* The same hook for the forms the plans launch (parity tests; not on the product path): one descriptor.  Every field of
 * ccvpe_op_conv2d keeps its meaning; beyond them:
 *   in_ld     floats per input pixel, >= Cin and a multiple of 4 (0 = Cin): `in` is [B,H,W,in_ld], channels past Cin are not read.
 *   gate      [B][Cin] device floats or NULL: the input is multiplied by gate[b][c] (squeeze-excite).  1x1 / stride 1 / pad 0
 *             convs only.
 *   resid     [B*OH*OW][resid_ld] device floats or NULL (resid_ld >= Cout), added to the result.  act must be 0: no plan adds a
 *             residual behind an activation, and the hook defines no order for it.  Not with CCVPE_OP_DECONV.
 *   dst, ndst 1 .. 3 destinations the caller allocates: destination i is [output pixels][ld], the Cout channels land at
 *             [coff, coff + Cout) of every row (coff + Cout <= ld), the other floats of a row are left alone.
 *   mode      CCVPE_OP_CONV, or CCVPE_OP_DECONV: ConvTranspose2d(kernel 2, stride 2), w [Cin,Cout,2,2] (KH = KW = stride = 2, pad 0),
 *             packed as a decoder level is (GEMM column (dy*2+dx)*Cout + o, 1x1 taps, pixel shuffle on store); 2H x 2W output pixels.
 *   ran_tile, ran_split, requested_runs   optional outputs: the tile id and split code the launcher recorded for the (first)
 *             launch - another tile than `tile & 255` means the requested one does not take this layer and the shape heuristic
 *             chose, split code 1 means K stayed whole, 64 + S that S slices reduced themselves - and whether the requested tile
 *             takes these launch parameters (1 / 0; -1 for tile id 0).  A Winograd id on a layer it does not take falls back
 *             like any other (ccvpe_op_conv2d refuses it).
 * Refusals (CCVPE_EINVAL, before any launch): those of ccvpe_op_conv2d; in_ld, resid_ld, ld / coff outside the ranges above; a
 * NULL destination; a gate or residual outside the uses above; any input, residual or destination of 2^31 elements or more.
 * Not expressible here: the squeeze-excite prologue of the latency-form project conv (se_rows) and the split-bf16 input and
 * destinations of the bf16x3 hand-off. */
enum { CCVPE_OP_CONV = 0, CCVPE_OP_DECONV = 1 };
typedef struct ccvpe_op_conv_dst { float* ptr; int32_t ld, coff; } ccvpe_op_conv_dst;
typedef struct ccvpe_op_conv_desc {
    const float* in;
    int32_t B, H, W, Cin, in_ld;
    const float* w;
    const float* bias;
    int32_t Cout, KH, KW, stride, pad, act, tile, mode;
    const float* gate;
    const float* resid;
    int32_t resid_ld, ndst;
    ccvpe_op_conv_dst dst[3];
    int32_t iters;
    float* ms;
    int32_t* ran_tile;
    int32_t* ran_split;
    int32_t* requested_runs;
} ccvpe_op_conv_desc;
int ccvpe_op_conv2d_ex(const ccvpe_op_conv_desc* d, void* stream);

/* Kernel-level hook for parity tests (not on the product path): the fused last decoder level on its own,
 * ConvTranspose2d(k2, s2, Cin -> 16) -> conv3x3(16 -> 16, pad 1) + ReLU -> conv3x3(16 -> Cout, pad 1), and for Cout == 2 the L2
 * normalisation over the channel (F.normalize, eps 1e-12).  H x W is the OUTPUT size (multiples of 16).  score != 0: channel 0 of the
 * Cin reference channels is a score channel, and `in` is the plan's padded layout [B, H/2, W/2, 8 + (Cin - 1)] = [score, 7 unused,
 * Cin - 1 descriptor channels]; score == 0: in [B, H/2, W/2, Cin].  The descriptor channel count is a multiple of 4, and at most 64
 * channels reach the kernel.  Weights and biases in the reference's layouts, host or device: wd [Cin,16,2,2], bd [16], wa [16,16,3,3],
 * ba [16], wt [Cout,16,3,3], bt [Cout]; they are composed by the code that serves ccvpe_create.  tile: 0 = 16 x 16 output tiles, 1 = 32
 * wide x 16 high where W is a multiple of 32 (16 x 16 otherwise); every tile gives every output the same bits.  tile word = id |
 * (workgroup cap << 8): a cap (>= 8) makes a small problem run the kernel's loop over tiles; 0 = the persistent grid.  out [B,Cout,H,W]
 * (device, NCHW).  Returns the tile that ran (0 or 1), or a negative error code. */
int ccvpe_op_level1(const float* in, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t score, const float* wd, const float* bd,
                    const float* wa, const float* ba, const float* wt, const float* bt, int32_t Cout, int32_t tile, float* out, void* stream);

/* Kernel-level hook for parity tests (not on the product path): deconv_k2s2_kernel on its own - ConvTranspose2d(k2, s2, Cin -> Cout) of
 * in [B, H, W, in_ld] (device, NHWC; the first Cin channels are the layer's input, in_ld >= Cin) into channels [coff, coff + cw) of out
 * [B, 2H, 2W, ld] (device, NHWC; nothing else of it is written).  cw >= Cout: the channels from coff + Cout on are written as zeros, as
 * a plan's concat buffer has them.  w [Cin,Cout,2,2] and bias [Cout] (or null) in the reference's layouts, host or device; they are
 * packed by the code that serves ccvpe_create.  Input channels whose weights are all zero are never multiplied: whatever `in` holds
 * there (NaN included) leaves the result alone.  Sizes the kernel does not take (Cin a multiple of 8; cw a multiple of 16 up to 80; in_ld,
 * ld, coff multiples of 4; at most 192 input channels with a weight that is not zero; the weights of two taps within the LDS) are
 * refused with CCVPE_EINVAL.  Returns the taps a workgroup holds (4: every input row is read once; 2: twice), or a negative error code. */
int ccvpe_op_deconv_k2s2(const float* in, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t in_ld, const float* w, const float* bias, int32_t Cout,
                         float* out, int32_t ld, int32_t coff, int32_t cw, void* stream);

/* Kernel-level hook (tests): the launches ccvpe_localize runs behind its decoders - softmax partials, the argmax without a prior,
 * posterior or summary, the orientation gather - on logits [batch][512*512] and ori [batch][2][512][512] the caller holds: rows
 * [batch][5], DEVICE memory, the bits ccvpe_postprocess_rows gives on ccvpe_forward's heatmap of those logits.  ccvpe_postprocess_prior
 * refuses a null prior and ccvpe_track_update_logits stores a map, so no other entry runs this form on given logits.  batch <= 4096,
 * any handle, the scratch of ccvpe_postprocess_prior. */
int ccvpe_op_pose_rows(ccvpe_handle h, const float* logits, const float* ori, int32_t batch, float* rows, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CCVPE_H */
