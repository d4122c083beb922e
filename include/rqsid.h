/*
 * rqsid.h — C ABI of the MI355X (gfx950) residual-quantisation semantic-ID kernels.
 *
 * The reference (zeehu/generative_ranking_recommender) has no FFI: its hot path
 * is the Python module API of balancekmeans / hierarchical_rq_kmeans /
 * simplified_semantic_id_generator, whose arithmetic is stock PyTorch ops.
 * Each entry point below replaces one of those op sequences; the reference
 * file:line it stands in for is cited per function.  The Python mirror of the
 * reference classes (generative_ranking_recommender_amd/) binds these with
 * ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (e.g. torch
 *    tensor.data_ptr()); nothing is allocated inside except what the caller
 *    passes as `workspace` (size from the matching *_workspace_bytes query);
 *  - all work is stream-ordered on the caller's hipStream_t (passed as void*),
 *    no host synchronisation, graph-capturable;
 *  - return 0 on success, a negative RQSID_E* code otherwise; the text of the
 *    last error of the calling thread is in rqsid_last_error();
 *  - matrices are row-major [rows][dim], fp32 unless an entry point says otherwise (rqsid_assign_x also
 *    takes the row matrix as IEEE fp16 or bfloat16); dim must be a multiple of 32.
 */
#ifndef RQSID_H
#define RQSID_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RQSID_OK 0
#define RQSID_E_ARG (-1)      /* bad argument (shape, null pointer, unsupported dim) */
#define RQSID_E_LAUNCH (-2)   /* HIP launch / runtime error */
#define RQSID_E_WORKSPACE (-3)

/* segment flags (rqsid_assign seg_flags[s]) */
#define RQSID_SEG_PENALTY 1u  /* empty allowed set: argmin over ALL centres of fl(d + 10000) */

/* row formats (rqsid_assign_x x_format) */
#define RQSID_X_F32 0   /* float */
#define RQSID_X_F16 1   /* IEEE binary16 */
#define RQSID_X_BF16 2  /* bfloat16 */

int rqsid_version(void);
const char* rqsid_last_error(void);
/* 0 for a product build; else the bits of the timing-probe macros it was compiled with (tools/ab_build.sh:
 * 1 RQSID_AB_MODE, 2 RQSID_AB_HALFROW, 4 RQSID_AB_NOROWDMA, 8 RQSID_AB_EPI, 16 RQSID_STAMPS,
 * 32 RQSID_AB_NO_FLUSH) -- such a library returns wrong IDs by design and must never ship. */
int32_t rqsid_build_flags(void);

/* Centre preparation for rqsid_assign.  The table is scaled by a power of two 2^s (largest element
 * just below 2^14) and split into two fp16 terms: hi = fp16(c 2^s) and lo = fp16((c 2^s - hi) 2^12),
 * scaled values outside the fp16 normal range stored as 0 (the MFMA must never see a subnormal).
 * c16 [k][dim/32][2][32] (IEEE half bits: per centre and 32-dim chunk, 32 hi terms then 32 lo terms,
 * one 128-B piece); c_meta [k+1][4]: row j <  k =
 * {|c|^2, |c|, |c - (hi + lo 2^-12) 2^-s|, |c - hi 2^-s|} (fp64-accumulated, feeding the screening
 * error bound), row k = {2^-s, max_j |c - (hi + lo 2^-12) 2^-s| / |c|, max_j |c - hi 2^-s| / |c|,
 * max_j |c|} (rounded up; the single-pass screens collapse their per-candidate bound onto |c|).  Replaces the per-call centre side of torch.cdist's
 * mm-expansion (ATen _euclidean_dist) used by pairwise_distance_full,
 * balancekmeans/__init__.py:576-603. */
int rqsid_prepare_centers(const float* centers, int64_t k, int32_t dim,
                          uint16_t* c16, float* c_meta, void* stream);
/* The hi terms of a prepared table alone, c16_hi [k][dim] fp16 (1 KiB per 512-d centre): the 1-term streamed
 * screens (the ping-pong and row-resident forms) gather their 64-B centre pieces from it when rqsid_assign
 * gets it, touching half the cache lines of the interleaved table (the XL last level's 5120 candidates: 5 MB
 * instead of 10 MB against a 4-MB XCD L2). */
int rqsid_prepare_centers_hi(const uint16_t* c16, int64_t k, int32_t dim, uint16_t* c16_hi, void* stream);

/* Counting sort of rows by segment key (keys in [0, n_segments)).
 * Outputs seg_row_off[S+1], seg_tile_off[S+1] (exclusive scan of
 * ceil(rows_in_segment / tile_rows)), row_index[n] (rows grouped by key).
 * Replaces the per-parent torch.where/mask loops of
 * hierarchical_rq_kmeans.py:711,880-885,1210-1216 and
 * simplified_semantic_id_generator.py:112,154-158,263.
 * Workspace int 2*n_segments (the first int after counts and cursors) is a sticky error word the
 * caller zeroes when it allocates the workspace (a call never clears it): every row_index write takes
 * its position from a device counter, and a position outside its key's segment drops the write and
 * sets bit 1 there (a wrong count can only report an error, never store outside row_index). */
int64_t rqsid_bucket_workspace_bytes(int64_t n, int32_t n_segments);
int rqsid_bucket(const int32_t* keys, int64_t n, int32_t n_segments, int32_t tile_rows,
                 int32_t* seg_row_off, int32_t* seg_tile_off, int32_t* row_index,
                 void* workspace, int64_t workspace_bytes, void* stream);

/* Rows per work tile of rqsid_assign (the tile_rows to pass to rqsid_bucket). */
int32_t rqsid_assign_tile_rows(void);

/* Segmented nearest-centre assignment (exact argmin, lowest index on ties).
 *
 * Segment s owns rows row_index[seg_row_off[s] .. seg_row_off[s+1]) (row_index
 * NULL = identity) and candidates j = 0 .. cand_count[s]-1 whose global centre
 * index is cand_idx[cand_base[s]+j] (cand_idx NULL: cand_base[s]+j).
 * out_local[row] = cand_lid[cand_base[s]+j] (cand_lid NULL: j) of the nearest allowed
 * centre, out_global[row] = its global index.  (A list may omit bitwise duplicates of an
 * earlier entry -- they can never be the first minimum -- and report the original local
 * ids through cand_lid.)  Segments flagged RQSID_SEG_PENALTY reproduce the reference's +10000
 * mask with an empty allowed set (argmin over all n_centers of fl32(d)+10000);
 * their out_local is -1.
 *
 * Replaces pairwise_distance_full + torch.argmin (balancekmeans/__init__.py:
 * 489-534, 576-603), the +10000-masked reassignment/prediction of
 * hierarchical_rq_kmeans.py:839-966,1146-1305 and the +inf-masked ones of
 * simplified_semantic_id_generator.py:145-161,305-331.
 *
 * Fused residuals (res_levels 1/2, one dimension group): the vector assigned for row i of
 * segment s is
 *   0: x_i
 *   1: u = x_i - ca[seg_ca[s]]             [ / (||u|| + 1e-8), written to den_out[i] ]
 *   2: v = (x_i - ca[seg_ca[s]])[/den_in[i]] - cb[seg_cb[s]]   [ / (||v|| + 1e-8) ]
 * (seg_ca NULL = identity), exactly the fp32 operation sequence of
 * _compute_residuals_with_centers (hierarchical_rq_kmeans.py:1088-1128, res_normalize=1) or of
 * the simplified generator's plain residuals (:91,167, res_normalize=0), without materialising
 * the residual matrix.  The residual centres are per SEGMENT: a level's segment (parent cluster,
 * (l1,l2) group) determines the parent IDs whose centres are subtracted.
 *
 * Method: fp16 MFMA screening (v_mfma_f32_32x32x16_f16) with a rigorous per-candidate error
 * bound, then an fp64 re-score of every row whose bound admits more than one candidate.
 * screen_terms: 1 = vh.ch only; 3 = vh.ch + vl.ch + vh.cl (both operands' fp16 rounding
 * residuals, a ~5x tighter bound for 3x the MFMA work; segments of <= 128 candidates only, wider
 * ones use 1); 0 = automatic (3 for residual levels with <= 128 candidates per segment); 2 = the 2-term
 * pairwise form of rqsid_assign_pair (below; RQSID_E_ARG here, where no pair table comes with the call).  The
 * result never depends on it, only the speed.
 *
 * Errors: RQSID_E_ARG / RQSID_E_WORKSPACE before any launch; RQSID_E_LAUNCH for a HIP launch failure
 * or, on the opt-in centre-resident screen (RQSID_SCREEN_VARIANT=6), when a wave's capped role wait
 * gave up (device error word read back after the call; the IDs it left are not returned as valid).
 * c16_hi: NULL or rqsid_prepare_centers_hi's table of the same centres (only where-from changes, never the IDs).
 * Workspace bytes [240, 244) are a sticky error word the caller zeroes when it allocates the workspace
 * (every call zeroes only [0, 240)): each list write whose index comes from a device counter (the
 * re-score compaction, the overflow list) is bounded by its slot's capacity, and a write that would fall
 * outside sets a bit here instead (1 compaction, 2 overflow list, 4 a list entry outside [0, n_rows),
 * 8 a device tile count past the tile maps / descriptors of the streamed, producer/consumer, row- and
 * centre-resident screens: clamped to their capacity). */
int64_t rqsid_assign_workspace_bytes(int64_t n_rows);
int rqsid_assign(const float* x, int64_t n_rows, int32_t dim, const int32_t* row_index,
                 int32_t n_segments, const int32_t* seg_row_off, const int32_t* seg_tile_off,
                 int64_t max_tiles,
                 const float* centers, const uint16_t* c16, const uint16_t* c16_hi, const float* c_meta,
                 int32_t n_centers,
                 const int32_t* cand_base, const int32_t* cand_count, int32_t cand_count_max,
                 const int32_t* cand_idx, const int32_t* cand_lid, const uint8_t* seg_flags,
                 int32_t res_levels, int32_t res_normalize,
                 const float* ca, const int32_t* seg_ca, const float* cb, const int32_t* seg_cb,
                 const float* den_in, float* den_out,
                 int32_t* out_local, int32_t* out_global, int32_t screen_terms,
                 void* workspace, int64_t workspace_bytes, void* stream);
/* rqsid_assign with the row matrix x in the format x_format (RQSID_X_*); every other argument as above, and the
 * same workspace query.  RQSID_X_F32 is rqsid_assign itself (the same dispatch).  RQSID_X_F16 / RQSID_X_BF16
 * read 16-bit rows [rows][dim] (x 16-byte aligned) with no fp32 copy of them anywhere: the screen streams
 * 64-B row pieces, widens each element to fp32 (lossless) as it leaves LDS and runs the fp32 operation
 * sequence from there, and the re-screen / re-score widen as they load, so the IDs (and den_out) are
 * bit-identical to rqsid_assign on the widened rows.  16-bit rows always take the per-tile screen (multi-pass
 * for segments wider than 256 candidates, or 128 with 3 terms): the streamed, producer/consumer, row- and
 * centre-resident screens and the candidate split are fp32-row kernels, so RQSID_SCREEN_VARIANT values that
 * name them (5, 6, 7, 8, 9) and RQSID_PC are ignored for these formats.  An unknown x_format is
 * RQSID_E_ARG before any launch. */
int rqsid_assign_x(const void* x, int32_t x_format, int64_t n_rows, int32_t dim, const int32_t* row_index,
                   int32_t n_segments, const int32_t* seg_row_off, const int32_t* seg_tile_off,
                   int64_t max_tiles,
                   const float* centers, const uint16_t* c16, const uint16_t* c16_hi, const float* c_meta,
                   int32_t n_centers,
                   const int32_t* cand_base, const int32_t* cand_count, int32_t cand_count_max,
                   const int32_t* cand_idx, const int32_t* cand_lid, const uint8_t* seg_flags,
                   int32_t res_levels, int32_t res_normalize,
                   const float* ca, const int32_t* seg_ca, const float* cb, const int32_t* seg_cb,
                   const float* den_in, float* den_out,
                   int32_t* out_local, int32_t* out_global, int32_t screen_terms,
                   void* workspace, int64_t workspace_bytes, void* stream);

/* Pair table of a level's segment lists, for rqsid_assign_pair: per segment s and list positions j, k <
 * cand_count[s] (cand_count_max <= 128), an fp16 upper bound of |c_j - c_k| (fp64 from the fp32 centres, rounded
 * up; in units of the centre table's scale, so build it after rqsid_prepare_centers of the same c_meta, and again
 * whenever the centres or the lists change).  pair_table: rqsid_pair_table_bytes(n_segments) bytes (32 KiB per
 * segment), 16-byte aligned; its layout is the screen's own. */
int64_t rqsid_pair_table_bytes(int32_t n_segments);
int rqsid_pair_table(const float* centers, int32_t dim, const float* c_meta, int32_t n_centers, int32_t n_segments,
                     const int32_t* cand_base, const int32_t* cand_count, int32_t cand_count_max,
                     const int32_t* cand_idx, uint16_t* pair_table, void* stream);
/* rqsid_assign_x with an optional pair table (NULL: rqsid_assign_x itself).  With one, and where the per-tile
 * single-pass 3-term screen of fp32 rows would run (segments of <= 128 candidates), its 2-term pairwise form
 * runs instead: vh.ch + vh.cl, the rows' own fp16 rounding charged per candidate pair as |x - fp16(x)| |c_k -
 * c_b| against the row's best candidate b.  One MFMA of three less; a few more rows reach the
 * re-score; the IDs are the same.  screen_terms = 2 asks for this form (RQSID_E_ARG without a table; the 3-term
 * screen where the form does not apply), 0 picks it wherever 3 terms would be picked, 3 and RQSID_NO_PAIR=1 keep
 * the 3-term screen.  rqsid_assign_plan_pair: 1 if a call of that shape, under the current environment, runs
 * the 2-term pairwise form. */
int rqsid_assign_pair(const void* x, int32_t x_format, int64_t n_rows, int32_t dim, const int32_t* row_index,
                      int32_t n_segments, const int32_t* seg_row_off, const int32_t* seg_tile_off,
                      int64_t max_tiles,
                      const float* centers, const uint16_t* c16, const uint16_t* c16_hi, const float* c_meta,
                      int32_t n_centers,
                      const int32_t* cand_base, const int32_t* cand_count, int32_t cand_count_max,
                      const int32_t* cand_idx, const int32_t* cand_lid, const uint8_t* seg_flags,
                      int32_t res_levels, int32_t res_normalize,
                      const float* ca, const int32_t* seg_ca, const float* cb, const int32_t* seg_cb,
                      const float* den_in, float* den_out,
                      int32_t* out_local, int32_t* out_global, int32_t screen_terms,
                      void* workspace, int64_t workspace_bytes, void* stream, const uint16_t* pair_table);
int32_t rqsid_assign_plan_pair(int32_t x_format, int64_t n_rows, int32_t dim, int32_t n_segments,
                               int32_t cand_count_max, int32_t res_levels, int32_t res_normalize,
                               int32_t screen_terms, int32_t has_cand_lid, int32_t has_den_out, int32_t has_pair);

/* The k nearest allowed centres of every row, exactly: rqsid_assign's question asked for the first k places.
 * Segments, tiles (rqsid_bucket with rqsid_assign_tile_rows()), candidate lists, x_format and the fused residual
 * chain (res_levels, res_normalize, ca / seg_ca, cb / seg_cb, den_in, den_out) mean exactly what they mean for
 * rqsid_assign_x, so the same tables serve both calls; den_out (res_levels 1, res_normalize) receives
 * fl32(sqrt(fp64 sum)) + 1e-8f as there.  The row's vector v is built with the fp32 operation sequence of
 * rqsid_assign's exact re-score (bit-identical to rqsid_residual's rows at res_levels 0).
 * Outputs, all [n_rows][k] row-major and indexed by row: slot t of a row of segment s holds the allowed centre with
 * the t-th smallest key (d2, position in the segment's list), d2 = sum_i ((double)v_i - (double)c_i)^2:
 * out_dist = fl32(sqrt(d2)), out_local = cand_lid[cand_base[s] + position] (cand_lid NULL: the position), out_global =
 * the centre row.  A list is ranked as given: bitwise-duplicate centres each take their place (pass the list
 * BEFORE any removal of duplicates).  Slot 0 therefore equals rqsid_assign's out_local / out_global on every row
 * whose distances are finite and whose segment is not a penalty segment.
 *  - slots t >= cand_count[s]: -1 / -1 / +inf;
 *  - a segment flagged RQSID_SEG_PENALTY has no allowed centre to rank: every slot of its rows -1 / -1 / +inf;
 *  - a row with a non-finite element of v, or a non-finite distance: -1 / -1 / NaN in every slot; it is counted
 *    (below) and is not an error.
 * Limits: 1 <= k <= RQSID_TOPK_MAX; dim % 32 == 0, dim <= 1024; x and centers 16-byte aligned; n_rows == 0 succeeds
 * without touching anything.  RQSID_E_ARG / RQSID_E_WORKSPACE before any HIP call.  Stream-ordered, no host
 * synchronisation, graph-capturable, no float atomics: two calls on the same inputs give identical bytes.
 * Method: per 128-row tile an fp32 screen on v_mfma_f32_32x32x2_f32 with a rigorous interval per
 * candidate, a per-row list of the candidates whose lower end does not exceed the k-th smallest upper end, and an
 * fp64 pass over the list; a row whose list overflows (many exact ties) takes the fp64 pass over all its candidates.
 * The result never depends on the interval's width, only the amount of fp64 work.
 * Workspace (rqsid_assign_topk_workspace_bytes; every list lives in LDS, so it is the header alone):
 *   bytes [0, 4)   sticky error word, zeroed by the caller at allocation and never cleared by a call.  No write of
 *                  this entry point takes its position from a device counter; the word records indices read from
 *                  device tables that were clamped instead of followed: 1 = the tile count seg_tile_off[n_segments]
 *                  exceeded max_tiles (the tiles beyond are not processed), 2 = a row position or row_index entry
 *                  outside [0, n_rows) (skipped), 4 = a candidate's centre row outside [0, n_centers) (centre row 0
 *                  is read instead; no address is formed from it);
 *   bytes [4, 16)  three int32 counters zeroed by every call: rows ranked from their list, rows that took the
 *                  all-candidate pass, non-finite rows. */
#define RQSID_TOPK_MAX 8
int64_t rqsid_assign_topk_workspace_bytes(int64_t n_rows, int32_t k);
int rqsid_assign_topk(const void* x, int32_t x_format, int64_t n_rows, int32_t dim, const int32_t* row_index,
                      int32_t n_segments, const int32_t* seg_row_off, const int32_t* seg_tile_off, int64_t max_tiles,
                      const float* centers, const float* c_meta, int32_t n_centers,
                      const int32_t* cand_base, const int32_t* cand_count, int32_t cand_count_max,
                      const int32_t* cand_idx, const int32_t* cand_lid, const uint8_t* seg_flags,
                      int32_t res_levels, int32_t res_normalize,
                      const float* ca, const int32_t* seg_ca, const float* cb, const int32_t* seg_cb,
                      const float* den_in, float* den_out,
                      int32_t k, int32_t* out_local, int32_t* out_global, float* out_dist,
                      void* workspace, int64_t workspace_bytes, void* stream);

/* Beam-search encode, step 1: rqsid_assign_topk over n_items = n_rows * beam items, item-major
 * (item = row * beam + h is hypothesis h of a row).  Every argument means what it means for rqsid_assign_topk (the
 * same kernel, instantiated for items), with three differences:
 *  - item i reads row i / beam of x: x keeps n_items / beam rows in any x_format, and no residual or replicated
 *    matrix is written.  row_index, the segments and tiles (rqsid_bucket over the items' keys), every output
 *    ([n_items][k]) and the counters count items;
 *  - den_in is indexed by item;
 *  - den_out (when given and res_normalize) receives the level's own divisor fl32(sqrt(fp64 sum)) + 1e-8f at
 *    res_levels 1 AND 2, indexed by item.
 * A dead hypothesis is an item like any other: the caller buckets it into one extra segment with cand_count = 0
 * (every slot -1 / -1 / +inf) whose seg_ca / seg_cb entries name row 0.
 * n_items % beam == 0 and 1 <= beam <= RQSID_TOPK_MAX; the other limits, the refusals before any HIP call, the
 * workspace header (sticky error word, three counters) are those of rqsid_assign_topk.  With beam = 1 the outputs
 * are byte-identical to rqsid_assign_topk on the same tables. */
int64_t rqsid_beam_expand_workspace_bytes(int64_t n_items, int32_t k);
int rqsid_beam_expand(const void* x, int32_t x_format, int64_t n_items, int32_t beam, int32_t dim,
                      const int32_t* row_index,
                      int32_t n_segments, const int32_t* seg_row_off, const int32_t* seg_tile_off, int64_t max_tiles,
                      const float* centers, const float* c_meta, int32_t n_centers,
                      const int32_t* cand_base, const int32_t* cand_count, int32_t cand_count_max,
                      const int32_t* cand_idx, const int32_t* cand_lid, const uint8_t* seg_flags,
                      int32_t res_levels, int32_t res_normalize,
                      const float* ca, const int32_t* seg_ca, const float* cb, const int32_t* seg_cb,
                      const float* den_in, float* den_out,
                      int32_t k, int32_t* out_local, int32_t* out_global, float* out_dist,
                      void* workspace, int64_t workspace_bytes, void* stream);

/* Beam-search encode, step 2: per row, the next beam out of the beam_in * k expansions of its beam_in hypotheses
 * (beam_in = 1 at level 0, where the expansions are rqsid_assign_topk's).  Inputs, by input item = row * beam_in + h:
 * exp_local / exp_global / exp_dist [n_rows * beam_in][k] (rqsid_beam_expand's outputs); scale_in = S_{l-1} and den =
 * the level's divisor den_l (either may be NULL, meaning 1); path_in [n_rows * beam_in][level] (NULL at level 0).
 * use_global != 0 takes exp_global as the level's id, else exp_local.
 * An expansion (h, place) with ids >= 0 scores rec = fl32(S_l d), S_l = fl32(scale_in[h] den[h]), d its exp_dist:
 * the original-space error of the path up to this level.  It is live when rec is finite.  Output slot 0 is always
 * (h = 0, place = 0), the greedy continuation (dead if that expansion is not live); slots 1 .. beam_out - 1 are the
 * other live expansions in ascending (rec, h, place) order; slots nothing fills are dead.  Outputs, by output item
 * row * beam_out + t: path_out [level + 1] (the parent's prefix, then the id); scale_out = S_l of the parent;
 * den_next = den of the parent (the next level's den_in); rec_out; key_out = (level >= 1 ? path_in[h][level - 1] *
 * key_mult : 0) + id (the next level's segment key); src_out = h * k + place.  A dead slot: ids -1, scale_out 1,
 * den_next 1, rec_out +inf, key_out = dead_key, src_out -1.  A row with a NaN exp_dist or a NaN scale_in in any input
 * item (a non-finite row): every slot dead with rec_out = scale_out = NaN, so the NaN reaches the last level.  The
 * den of an item without a live expansion never reaches an output (rqsid_beam_expand leaves it unwritten for the
 * items of a penalty segment).
 * One wave per row, no atomics, no device-counter-driven writes: a pure function of its inputs, bit-reproducible,
 * stream-ordered, graph-capturable.  RQSID_E_ARG before any launch: beam_in, k, beam_out outside 1 .. RQSID_TOPK_MAX,
 * beam_out > beam_in * k, level outside 0 .. 7, more than 2^31 - 1 items, a null required pointer (every output, the
 * expansions, path_in at level >= 1).  n_rows == 0 succeeds without touching anything. */
int rqsid_beam_merge(int64_t n_rows, int32_t beam_in, int32_t k, int32_t beam_out, int32_t level,
                     const int32_t* exp_local, const int32_t* exp_global, const float* exp_dist,
                     const float* scale_in, const float* den, const int32_t* path_in,
                     int32_t use_global, int32_t key_mult, int32_t dead_key,
                     int32_t* path_out, float* scale_out, float* den_next, float* rec_out,
                     int32_t* key_out, int32_t* src_out, void* stream);

/* Residual r = x - c[center_id[row]]; with normalize != 0 each dimension group
 * g is divided by (||r_g|| + 1e-8).  Replaces _compute_residuals_with_centers
 * (hierarchical_rq_kmeans.py:1088-1128) and the plain residuals of
 * simplified_semantic_id_generator.py:78-96,164-168. */
int rqsid_residual(const float* x, int64_t n, int32_t dim, const float* centers, int32_t n_centers,
                   const int32_t* center_id, const int32_t* group_dims, int32_t n_groups,
                   int32_t normalize, float* out, void* stream);

/* Quantisation error of an encoding: one streaming pass that rebuilds the residual chain of IDs that are already
 * chosen, with the fp32 operation sequence of _compute_residuals_with_centers (hierarchical_rq_kmeans.py:1088-1128,
 * res_normalize != 0) or of the simplified generator's plain residuals (simplified_semantic_id_generator.py:78-96,
 * 164-168, res_normalize == 0), one dimension group:
 *   r0 = x - c0[id0];  e0 = fl32(sqrt(sum (double)r0_i^2));  v1 = res_normalize ? r0 / (e0 + 1e-8f) : r0;
 *   r1 = v1 - c1[id1]; e1 likewise; ...
 * so e_l is the distance from level l's input vector to its assigned centre, and e_l + 1e-8f the next level's
 * divisor (the den_out of rqsid_assign's fused level 1).  x: [n_rows][dim] in x_format (RQSID_X_*, 16-byte aligned,
 * 16-bit rows widened as they load: no fp32 copy); dim % 32 == 0, dim <= 1024; n_levels 1..3, levels beyond it take
 * NULL / 0.  idL[row] is the GLOBAL row of cL assigned to that row (indexed by row).  row_order: NULL or a
 * permutation of the rows that only sets the order they are processed in (e.g. rqsid_bucket's row_index by the last
 * level's group: centre rows of the earlier levels are then re-read once per group); no per-row output depends on it.
 * Outputs: err [n_levels][n_rows] level-major (required); x_norm [n_rows] = fl32(sqrt(sum (double)x_i^2)) (may be
 * NULL); sums double[n_levels + 1] (may be NULL) = per level the sum over rows of (double)e_l^2, then the sum of
 * (double)x_norm^2, added in a fixed order (per-block partials in the workspace, then a one-block kernel: no float
 * atomics), bit-identical between two calls with the same inputs and row_order.
 * A row whose id at some level is outside [0, kL) reads centre row 0 there instead (no address is formed from the
 * id), gets NaN in err at that level and every later one, and is left out of every entry of sums.
 * Workspace bytes [0, 4) are a sticky error word the caller zeroes when it allocates the workspace (a call never
 * clears it): value 1 = an id out of range, 2 = a row_order entry outside [0, n_rows) (that position is skipped).
 * RQSID_E_ARG / RQSID_E_WORKSPACE before any HIP call; n_rows == 0 succeeds and zeroes sums. */
int64_t rqsid_quant_error_workspace_bytes(int64_t n_rows);
int rqsid_quant_error(const void* x, int32_t x_format, int64_t n_rows, int32_t dim,
                      const int32_t* row_order,
                      int32_t n_levels, int32_t res_normalize,
                      const float* c0, int32_t k0, const int32_t* id0,
                      const float* c1, int32_t k1, const int32_t* id1,
                      const float* c2, int32_t k2, const int32_t* id2,
                      float* err, float* x_norm, double* sums,
                      void* workspace, int64_t workspace_bytes, void* stream);

/* Exact silhouette sums of scored rows against every cluster: the pairwise half of the reference's
 * quality check, sklearn's silhouette_score on the raw vectors (src/semantic_id_generator/calculate_metrics.py),
 * without materialising any distance matrix.
 * Cluster c is the set of rows row_index[seg_row_off[c] .. seg_row_off[c+1]) (row_index NULL = identity; the output
 * of rqsid_bucket over the labels serves as it is), n_c its size, d(i, j) the Euclidean distance.  Query i (row i of
 * q, [n_queries][dim] in x_format like x) has own cluster o = query_seg[i] (-1: none; query_seg NULL = all -1) and
 * self row r = query_self[i] (the row of x that IS this query, or -1; NULL = all -1):
 *   S(i, c) = sum over j in c, j != r, of d(i, j);
 *   a = S(i, o) / (n_o - 1) with a self row, S(i, o) / n_o without (0 when that divisor is 0, and when o = -1);
 *   b = min over non-empty c != o of S(i, c) / n_c, lowest c on an exact tie; out_b_seg = that c;
 *   s = (b - a) / max(a, b); 0 when max(a, b) = 0, and (sklearn's rule) 0 for a query with a self row whose own
 *   cluster has one row.  With o = -1 every cluster competes for b (the caller ignores s).  No other non-empty
 *   cluster: b = +inf, out_b_seg = -1, s = NaN.
 * The self row is excluded by INDEX, never by value (the expanded form below does not return 0 for d(i, i)).  A
 * non-finite value reaching a sum makes that query's a / b / s NaN (out_b_seg -1); it is not an error.
 * Arithmetic: d = fl32(sqrt(max(0, fl32(|q|^2 + |x_j|^2) - 2 D))) with D the dot product on v_mfma_f32_32x32x2_f32
 * (bitwise an fmaf chain over the dims in order; 3.1g's bound on |D - q.x| applies) and the squared norms
 * accumulated in fp64 and rounded once, as c_meta's.  Distances are added in fp32 inside one (tile, cluster) piece
 * of at most rqsid_silhouette_tile_rows() consecutive positions of the bucketed order, in position order; pieces,
 * chunks and the divisions are fp64, in a fixed order; a and b are rounded to fp32 once, at the store, and s is
 * formed from the fp64 values.  No float atomics: two calls with the same arguments return identical bytes, and
 * chunk_rows moves only fp64 roundings.  RQSID_X_F16 / RQSID_X_BF16 rows and queries are widened as they are staged
 * (no fp32 copy of them anywhere); the outputs are bit-identical to the call on the widened fp32 rows.
 * Limits: dim % 32 == 0, dim <= 1024; n_rows < 2^31; x and q 16-byte aligned; chunk_rows (base positions per block)
 * 0 = automatic (the fewest chunks that give 2048 blocks) or a positive multiple of the tile rows; n_queries == 0
 * or n_rows == 0 succeeds without touching anything.  RQSID_E_ARG / RQSID_E_WORKSPACE before any HIP call.
 * Stream-ordered, no host synchronisation, graph-capturable.
 * Workspace (rqsid_silhouette_workspace_bytes: the header, the squared norms of rows and queries, one 48-byte
 * record per query and chunk): bytes [0, 4) are a sticky error word the caller zeroes when it allocates the
 * workspace (a call never clears it): 1 = a row_index or query_self entry outside [0, n_rows) (query_self: other
 * than -1; the entry is skipped / taken as -1), 2 = a query_seg entry outside [-1, n_segments) (taken as -1), 4 = a
 * seg_row_off entry outside [0, n_rows] or decreasing (clamped into [0, n_rows]; positions no cluster owns are left
 * out).  No address is formed from an unchecked index: rows are addressed by position inside [0, n_rows) and by
 * row_index entries inside it, and the offsets only place boundaries. */
int32_t rqsid_silhouette_tile_rows(void);
int64_t rqsid_silhouette_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t chunk_rows);
int rqsid_silhouette(const void* x, int32_t x_format, int64_t n_rows, int32_t dim,
                     const int32_t* row_index, int32_t n_segments, const int32_t* seg_row_off,
                     const void* q, int32_t n_queries, const int32_t* query_self, const int32_t* query_seg,
                     int32_t chunk_rows, float* out_a, float* out_b, int32_t* out_b_seg, float* out_s,
                     void* workspace, int64_t workspace_bytes, void* stream);

/* The exact k nearest rows of every query, over all rows or inside one segment of the bucketed order (DESIGN.md
 * 3.3c): the batched form of the reference's Evaluator.find_neighbors (src/semantic_id_generator/
 * evaluate_semantic_ids.py) and the base of neighbourhood-preservation reports, without any distance matrix.
 * x, x_format, row_index, n_segments, seg_row_off, q, query_self and chunk_rows mean what they mean for
 * rqsid_silhouette (the output of rqsid_bucket serves as it is); n_segments == 0 with seg_row_off NULL is allowed:
 * every query is then unrestricted.  Query i searches the rows at positions [seg_row_off[s], seg_row_off[s+1]) of
 * the order when s = query_seg[i] >= 0, every row when s == -1 or query_seg is NULL; the row query_self[i] is
 * excluded by INDEX, never by value.
 * Key, in fp64 from the widened elements, lanes over 16-byte pieces and the re-score's halving reduction:
 *   RQSID_KNN_L2      d2 = sum((double) q_i - (double) x_i)^2, ascending; out_val = fl32(sqrt(d2));
 *   RQSID_KNN_COSINE  sim = dot / (sqrt(qq) sqrt(xx)), descending; out_val = fl32(sim).
 * Ties in the key go to the lowest ROW NUMBER of x: the output is a function of the row set alone, and chunk_rows
 * or a permutation of row_index inside segments leave every output byte unchanged.  out_row / out_val are
 * [n_queries][k]; slots beyond the number of eligible rows hold -1 / +inf.  A base row with a non-finite element
 * (cosine: or of zero norm) is never a neighbour; a query with a non-finite element (cosine: or of zero norm) gets
 * -1 / NaN in every slot and is counted.
 * Method: an fp32 screen on v_mfma_f32_32x32x2_f32 keeps the k + 8 smallest screen values per (query, chunk) with a
 * derived interval e >= |s - t|; a (query, chunk) pair whose list cannot be proven complete (more than 8 rows inside
 * the interval around the k-th place: true ties, duplicated rows; or a value outside the interval's premises) is
 * walked row by row in fp64.  e, the slack and chunk_rows move only the amount of fp64 work.
 * Limits: 1 <= k <= RQSID_KNN_MAX; dim % 32 == 0, dim <= 1024; n_rows < 2^31; x and q 16-byte aligned; chunk_rows 0
 * (automatic) or a positive multiple of rqsid_row_knn_tile_rows(); n_queries == 0 or n_rows == 0 succeeds without
 * touching anything.  RQSID_E_ARG / RQSID_E_WORKSPACE before any HIP call (a query_seg without seg_row_off is
 * RQSID_E_ARG).  Stream-ordered, no host synchronisation, graph-capturable; no float atomics; no write takes its
 * position from a device counter.
 * Workspace (rqsid_row_knn_workspace_bytes): bytes [0, 4) the sticky error word with rqsid_silhouette's three bits
 * (1, 2, 4; row_index is checked whole), zeroed by the caller once; bytes [4, 16) three int32 counters zeroed by every
 * call: queries ranked from their lists alone, (query, chunk) pairs that took the all-rows pass, queries without an
 * answer (non-finite / zero norm). */
#define RQSID_KNN_MAX 16
#define RQSID_KNN_L2 0
#define RQSID_KNN_COSINE 1
int32_t rqsid_row_knn_tile_rows(void);
int64_t rqsid_row_knn_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t k, int32_t chunk_rows);
int rqsid_row_knn(const void* x, int32_t x_format, int64_t n_rows, int32_t dim,
                  const int32_t* row_index, int32_t n_segments, const int32_t* seg_row_off,
                  const void* q, int32_t n_queries, const int32_t* query_self, const int32_t* query_seg,
                  int32_t metric, int32_t k, int32_t chunk_rows,
                  int32_t* out_row, float* out_val,
                  void* workspace, int64_t workspace_bytes, void* stream);

/* The exact k nearest rows of every query among the rows of a few position ranges of the order: the search through
 * the ID index.  x, x_format, row_index (position -> row, NULL = identity), q, query_self, metric and
 * k mean what they mean for rqsid_row_knn.  probe_lo / probe_hi are [n_queries][n_probes] half-open position ranges
 * (the cell index's order with its cell_off, or any rqsid_bucket output, serves as it is).  Query i searches the
 * UNION of its ranges; the result is the exact k nearest rows of that set with rqsid_row_knn's fp64 key, arithmetic,
 * tie rule (lowest row number of x), self exclusion by index, -1 / +inf past the eligible rows, and its rules for
 * rows and queries without a key.  With one range equal to a segment the outputs are byte-identical to rqsid_row_knn
 * with that query_seg, with [0, n_rows) to the unrestricted call.  The outputs are a function of the row SET: the
 * order of a query's probes, the order of the queries, a permutation of row_index inside ranges and added empty
 * ranges change no output byte.  out_scanned (may be NULL): per query the number of positions in its cleaned ranges.
 * Method: (query, probe) items, read in place, are ordered by the start of their range (rqsid_bucket's kernels; the
 * order decides only which items share a block); a block of up to 128 consecutive items merges their tile intervals into
 * runs and sweeps run after run with rqsid_row_knn's fp32 MFMA screen, each item limited to its range, keeping the
 * k + 8 smallest screen values per item; one fold per query over its items' lists, then the fp64 pass over what can
 * still place and over every row of an item whose list could not be proven complete.
 * Limits: 1 <= n_probes <= RQSID_PROBE_MAX; n_queries * n_probes < 2^31; the rest as rqsid_row_knn.  n_queries == 0
 * or n_rows == 0 succeeds without touching anything.  RQSID_E_ARG / RQSID_E_WORKSPACE before any HIP call.
 * Stream-ordered, no host synchronisation, graph-capturable; no float atomics; two calls on the same inputs give
 * identical output bytes.
 * Workspace (rqsid_probe_knn_workspace_bytes): bytes [0, 4) the sticky error word, zeroed by the caller once, never
 * by a call: 1 = a row_index / query_self entry outside the rows (skipped / taken as -1); 4 = a range end outside
 * [0, n_rows] or lo > hi (clamped; lo > hi is empty); 8 = two ranges of one query overlap (the one with the higher
 * probe index is dropped whole for that query).  Bytes [4, 20): four int32 counters zeroed by every call: queries
 * ranked from their lists alone, (query, probe) items that took the all-rows pass, queries without an answer, tile
 * visits of the screen. */
#define RQSID_PROBE_MAX 32
int64_t rqsid_probe_knn_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t n_probes, int32_t k);
int rqsid_probe_knn(const void* x, int32_t x_format, int64_t n_rows, int32_t dim,
                    const int32_t* row_index,
                    const void* q, int32_t n_queries, const int32_t* query_self,
                    int32_t n_probes, const int32_t* probe_lo, const int32_t* probe_hi,
                    int32_t metric, int32_t k,
                    int32_t* out_row, float* out_val, int32_t* out_scanned,
                    void* workspace, int64_t workspace_bytes, void* stream);

/* The ID cell index: which rows share a full ID, each row's place among them, and the collision
 * counters: the base of the reference's debug_collisions.py / analyze_semantic_ids.py figures, of
 * evaluate_semantic_ids.py's find_songs_by_semantic_id and of a disambiguating last token.
 * A cell is the set of rows with the same (group, fine ID).  Group g is the set of rows row_index[seg_row_off[g] ..
 * seg_row_off[g+1]) (row_index NULL = identity; the output of rqsid_bucket over every level but the last serves as it
 * is); fine_id[row] in [0, n_fine) is the last level (NULL: n_fine must be 1 and every group is one cell).
 * Order inside a cell: ascending (key, row number), the key being rank_key[row] mapped to a total order (-0 taken as
 * +0, every NaN after +inf); rank_key NULL: by row number alone.  The row number breaks every tie, so the output is a
 * function of the row set alone: a permutation of row_index inside segments changes no output byte, and two calls give
 * identical bytes.
 * Outputs by row: out_rank (place in its cell), out_size (size of its cell), out_cell (its cell's number among the
 * non-empty cells in (group, fine) order).  By position: out_order[n_rows], the rows in (group, fine, rank) order.  By
 * cell j < n_cells (capacity min(n_rows, n_groups * n_fine), one more for cell_off): cell_off[j] the position in
 * out_order where cell j starts, cell_off[n_cells] the end of the last cell (0 without cells), cell_group[j] and
 * cell_fine[j] its ID; entries past n_cells are not written.  Cells come out in lexicographic ID order, so an ID prefix
 * is a contiguous range of cells and of out_order.
 * A group flagged RQSID_CELLS_GROUP_SKIP in group_flags (NULL: none) forms no cells: its rows get -1 in rank, size and
 * cell, keep their row_index order in out_order and are counted nowhere.
 * Workspace (rqsid_id_cells_workspace_bytes): bytes [0, 4) the sticky error word, zeroed by the caller once: 1 = a
 * row_index entry outside [0, n_rows) (skipped; the group's span of out_order ends with one -1 per such entry), 2 = a
 * seg_row_off entry outside [0, n_rows] or decreasing (clamped), 4 = a fine_id outside [0, n_fine): the row goes to an
 * extra bin after its group's cells (in row order) and gets -1 / -1 / -1; no address is formed from the ID.  Bytes
 * [4, 152) are 37 int32 counters zeroed by every call: n_cells, cells of size >= 2, rows in such cells, cells of size
 * 1, the largest cell, and 32 bins counting the cells with size in [2^b, 2^(b+1)).
 * Limits: n_rows < 2^31, 1 <= n_fine <= RQSID_CELLS_FINE_MAX; n_rows == 0 succeeds without touching anything.
 * RQSID_E_ARG / RQSID_E_WORKSPACE before any HIP call.  Stream-ordered, no host synchronisation, graph-capturable.
 * Integer atomics only (LDS histograms and the counters); no write takes its position from a device counter: the
 * groups' cell counts are scanned by a kernel, and only the slot inside a cell's span comes from an LDS cursor, before
 * the ranking fixes the final order.
 * Method: per group an LDS histogram over the fine ID (groups of up to 1536 rows on one-wave blocks, up to 16384 on
 * 256 threads, 1024 threads beyond; only the n_fine + 1 counters live in LDS, so groups are unbounded), a scan of the
 * groups' cell counts, placement of the rows by cell into the workspace, then ranking per tile of 1024 positions, not
 * per group: the (key bits, row) words of the cells that start in the tile are ranked in LDS, by counting up to 384
 * rows and by a bitonic sort up to rqsid_id_cells_lds_rows(); a larger cell is sorted in runs of that size, written
 * to the workspace, each element's rank being the sum of its lower bounds in the runs (rows x runs x 10 reads for
 * one such cell, by one block: the price of a degenerate ID).
 * Measured on an MI355X with rqsid_bucket in front, against a stable torch sort of (cell key << 32 | key bits) with
 * unique_consecutive and the rank / size arithmetic (tools/id_cells_bench.py, profiles/id_cells_ab.json): 10M rows
 * of the bench's encode, 75,752 cells, 1.73 ms against 2.63 ms; 6.25M rows over 65,536 groups x 512, 5.28M cells,
 * 1.12 ms against 1.70 ms.  The tool's gate (at most half the composition's time) is NOT met: 0.66 at both shapes. */
#define RQSID_CELLS_FINE_MAX 8192
#define RQSID_CELLS_GROUP_SKIP 1u
int32_t rqsid_id_cells_lds_rows(void);   /* largest cell ranked inside LDS in one piece */
int64_t rqsid_id_cells_workspace_bytes(int64_t n_rows, int32_t n_groups, int32_t n_fine);
int rqsid_id_cells(int64_t n_rows, const int32_t* row_index, int32_t n_groups, const int32_t* seg_row_off,
                   const uint8_t* group_flags, const int32_t* fine_id, int32_t n_fine, const float* rank_key,
                   int32_t* out_order, int32_t* out_rank, int32_t* out_size, int32_t* out_cell,
                   int32_t* cell_off, int32_t* cell_group, int32_t* cell_fine,
                   void* workspace, int64_t workspace_bytes, void* stream);

/* The ID trie: the tables a generative retriever's constrained decoding walks, built from the cells
 * of rqsid_id_cells: the device form of the reference's SemanticIDTrie (src/generator/semantic_id_trie.py).
 * cell_group[n_cells] / cell_fine[n_cells] as rqsid_id_cells writes them (distinct, lexicographically ascending);
 * sizes[levels] (HOST array, required even without cells) the levels' sizes: the last level is the fine ID (at most
 * RQSID_CELLS_FINE_MAX), the group the mixed-radix number of the others (product at most 2^24); with one level, level
 * 0 is the group and the fine ID is 0.  keep[n_cells] (uint8, NULL = all): a cell with keep == 0 is not in the trie
 * (the reference never inserts a sequence with an unknown token).
 * A node of depth d (1 .. levels) is a distinct d-prefix among the kept cells, numbered from 0 in lexicographic order
 * per depth; the depth-levels nodes are the kept cells in order; the root is the one node of depth 0.
 * Outputs (int32, device; entries past the counts are not written):
 *   count[levels + 1]                 count[0] = 1, count[d] the nodes of depth d
 *   value[levels][n_cells]            value[d - 1][j] the level-(d - 1) ID value of depth-d node j
 *   child_off[levels][n_cells + 1]    child_off[d][j] the first depth-(d + 1) child of depth-d node j, and
 *                                     child_off[d][count[d]] = count[d + 1]; the children of a node ascend in value
 *   leaf_cell[n_cells]                the cell number of depth-levels node j (cell_off[leaf_cell[j]]: its rows)
 * Workspace (rqsid_id_trie_workspace_bytes): bytes [0, 4) the sticky error word, zeroed by the caller once: 1 = a cell
 * outside sizes, or not above the cell before it (cell i is compared with cell i - 1 as given); the cell is dropped.
 * The tables are nested and in bounds whatever the input, and are the kept cells' trie whenever those ascend.
 * Limits: n_cells < 2^31, 1 <= levels <= RQSID_TRIE_LEVELS_MAX; n_cells == 0 succeeds without touching anything (the
 * caller then holds count = {1, 0, ...} and child_off[d][0] = 0 itself).  RQSID_E_ARG / RQSID_E_WORKSPACE before any
 * HIP call.  Stream-ordered, no host synchronisation (the counts stay on the device; every grid is sized by n_cells),
 * graph-capturable.  Integer arithmetic only, no atomics but the error word's OR; no write position comes from an
 * input: each is a scan of flags, compared with the capacity.  Two calls give identical bytes.
 * Method: flag the cells, scan, compact the kept cells' IDs; flag per kept cell and depth "starts a node" (one bit per
 * depth in a byte), scan all depths at once, emit.  A scan is per-tile sums (2048 cells a block), one block over the
 * tile sums (a run of tiles per thread) and the consuming pass: 8 launches for any n_cells. */
#define RQSID_TRIE_LEVELS_MAX 8
int64_t rqsid_id_trie_workspace_bytes(int64_t n_cells, int32_t levels);
int rqsid_id_trie(int64_t n_cells, const int32_t* cell_group, const int32_t* cell_fine, int32_t levels,
                  const int32_t* sizes, const uint8_t* keep,
                  int32_t* count, int32_t* value, int32_t* child_off, int32_t* leaf_cell,
                  void* workspace, int64_t workspace_bytes, void* stream);

/* Constrained-decoding mask: the reference's ConstrainedLogitsProcessor.__call__ (_extract_current_prefix,
 * get_valid_next_tokens, masked_fill; src/generator/semantic_id_trie.py) for a whole batch in one call.
 * The trie: capacity (the n_cells the tables were built with: value is [levels][capacity], child_off [levels]
 * [capacity + 1]), levels, sizes (host), count, value, child_off.  input_ids [n_rows][n_tokens] with row stride ids_ld,
 * int32 (RQSID_IDS_I32) or int64 (RQSID_IDS_I64); n_tokens may be 0 (input_ids then NULL).  scores [n_rows][vocab]
 * with row stride ld >= vocab in elements, x_format RQSID_X_F32 / F16 / BF16, masked in place; the pointer and the
 * rows need only the element's alignment.  The token table: tok_code[vocab] = -1 for a token that is no ID token, else
 * level << 24 | value; level_tok[sum(sizes)], the levels one after another: the token number of (level, value) or -1;
 * eos in [0, vocab).  vocab <= RQSID_TRIE_VOCAB_MAX.
 * Per row: (1) the last position whose token has level 0 in tok_code starts the prefix (a token number outside
 * [0, vocab) is no ID token); without one the prefix is empty, else it is the tokens from there on, at most `levels`.
 * (2) a prefix of `levels` tokens (kind 1, complete): every level-0 token (level_tok[v] >= 0 for v < sizes[0], in the
 * trie or not) and eos are allowed.  (3) otherwise (kind 0) the trie is walked from the root: the token at place t
 * must have level t and its value be a child of the current node (binary search in the node's child range); the
 * tokens of the reached node's children are allowed.  (4) a failed walk or an empty allowed set (kind 2, dead): only
 * eos.  (5) scores[b][v] keeps its bytes for an allowed v (NaN included) and becomes -inf of the format for every other
 * v < vocab (NaN included); elements in [vocab, ld) are not touched.
 * Optional outputs per row (NULL: not wanted): out_kind, out_node (the node reached, -1 unless kind 0), out_count (the
 * allowed tokens; exact when level_tok names each token once and agrees with tok_code).
 * Workspace (rqsid_trie_mask_workspace_bytes): bytes [0, 4) the sticky error word, zeroed by the caller once: 1 = a
 * child range outside the counts (clamped), 2 = a level_tok entry outside [-1, vocab) (skipped).  Bytes [4, 16): three
 * int32 counters zeroed by every call: the rows of kind 0, 1, 2.
 * n_rows == 0 or vocab == 0 succeeds without touching anything.  RQSID_E_ARG / RQSID_E_WORKSPACE before any HIP call
 * (n_rows x ceil(vocab / 8192) must stay below 2^31).  Stream-ordered, no host read, graph-capturable; no float
 * atomics; no address is formed from an unchecked token number, child offset, value or level_tok entry; two calls on
 * the same inputs leave identical bytes.
 * Method: a walk kernel (one wave per row) writes each row's kind, prefix length and child range to the workspace; the
 * mask kernel (one block per 8192-element slice of a row) sets the allowed tokens of its slice in an LDS bitmap and
 * stores 16-byte pieces: a piece without an allowed token is stored without being read, one with only allowed tokens
 * is left alone, a mixed one is read, blended and stored; the row's unaligned head and tail go element by element. */
#define RQSID_TRIE_VOCAB_MAX 1048576
#define RQSID_IDS_I32 0
#define RQSID_IDS_I64 1
int64_t rqsid_trie_mask_workspace_bytes(int64_t n_rows);
int rqsid_trie_mask(int64_t capacity, int32_t levels, const int32_t* sizes, const int32_t* count,
                    const int32_t* value, const int32_t* child_off,
                    const void* input_ids, int32_t ids_format, int64_t n_rows, int32_t n_tokens, int64_t ids_ld,
                    void* scores, int32_t x_format, int32_t vocab, int64_t ld,
                    const int32_t* tok_code, const int32_t* level_tok, int32_t eos,
                    int32_t* out_kind, int32_t* out_node, int32_t* out_count,
                    void* workspace, int64_t workspace_bytes, void* stream);

/* One constrained beam step over trie nodes (no reference counterpart: the retrieval-style decode of the same trie,
 * carrying node numbers in place of token rows).  depth d in [0, levels); node_in [n_rows][beam_in] depth-d node
 * numbers (beam_in = 1 and node 0 at depth 0; a value outside [0, count[d]) is a dead hypothesis); score_in
 * [n_rows][beam_in] fp32 (NULL = 0); logp [n_rows * beam_in][ld] in x_format, ld >= vocab; level_tok as above.
 * A candidate is (h, c): a hypothesis h that is not dead and whose score_in is no NaN, and a child c of its node whose
 * token t = level_tok[d][value[c]] lies in [0, vocab).  Its score is s = fl32(score_in[h] + (float) logp[b beam_in +
 * h][t]); it is live unless s is NaN or -inf.  The output holds the first beam_out live candidates in the order (s
 * descending, h ascending, value ascending; -0 equals +0): node_out (depth d + 1), score_out, and, where wanted (NULL:
 * not), parent_out (h), value_out, token_out; unfilled slots hold -1 / -inf / -1 / -1 / -1.
 * beam_in, beam_out in 1 .. RQSID_TRIE_BEAM_MAX; a node's first 2^24 children are candidates.  n_rows == 0 succeeds
 * without touching anything; RQSID_E_ARG before any HIP call.  Stream-ordered, no workspace, no atomics, no write
 * position from a device counter; a pure function of its inputs, bit-reproducible.
 * Method: one block per batch row; every candidate has its own 64-bit key (the score's place in order above the
 * inverted (h, child rank)), each thread holds the largest key of its own candidates, and a round takes the block's
 * largest, after which only the thread that owned it looks through its candidates again.  64 x 8192 candidates per
 * row work, slowly (2048 candidates per thread and round for the owning thread). */
#define RQSID_TRIE_BEAM_MAX 64
int rqsid_trie_beam_step(int64_t capacity, int32_t levels, const int32_t* sizes, const int32_t* count,
                         const int32_t* value, const int32_t* child_off,
                         int32_t depth, int64_t n_rows, int32_t beam_in, int32_t beam_out,
                         const int32_t* node_in, const float* score_in,
                         const void* logp, int32_t x_format, int32_t vocab, int64_t ld, const int32_t* level_tok,
                         int32_t* node_out, float* score_out, int32_t* parent_out, int32_t* value_out,
                         int32_t* token_out, void* stream);

/* y = x * w_g per dimension group (hierarchical_rq_kmeans.py:583-604). */
int rqsid_scale_groups(const float* x, int64_t n, int32_t dim, const int32_t* group_dims,
                       int32_t n_groups, const float* weights, float* out, void* stream);

/* Lloyd centroid update, first half: per-cluster fp64 sums over the rows of
 * each segment (bucketed by rqsid_bucket with rqsid_centroid_tile_rows()).
 * sums must be zeroed by the caller.  Replaces the per-cluster
 * nonzero/index_select/mean loop of balancekmeans/__init__.py:315-324,434-443.
 * A row whose key lies outside [0, n_segments) is in no segment of rqsid_bucket's
 * tables, so it enters no sum and no count; the other clusters are unaffected.
 * Every sum is an fp64 sum of the cluster's fp32 rows in an unspecified order
 * (within count * 2^-52 * sum|x| of the exact sum), so the fp32 mean written by
 * rqsid_centroid_finalize is the correctly rounded mean up to that sliver. */
int32_t rqsid_centroid_tile_rows(void);
int rqsid_centroid_accumulate(const float* x, int32_t dim, const int32_t* row_index,
                              int32_t n_segments, const int32_t* seg_row_off,
                              const int32_t* seg_tile_off, int64_t max_tiles,
                              double* sums, void* stream);
/* Second half: centers[k] = fp32(sums[k] / count[k]) for count[k] > 0 (others
 * untouched; the caller fills empty clusters exactly as the reference does). */
int rqsid_centroid_finalize(const double* sums, const int32_t* seg_row_off, int32_t k,
                            int32_t dim, float* centers, void* stream);

/* Match matrix (uint8 [groups][n_cand], 1 = allowed) to candidate lists:
 * cand_count[g] = row popcount, cand_base[g] = exclusive scan, cand_idx = allowed
 * columns in ascending order (so the local index IS the remapped id of
 * _merge_match_matrix_cluster_ids, hierarchical_rq_kmeans.py:1055-1086),
 * seg_flags[g] = RQSID_SEG_PENALTY for empty rows. cand_idx needs
 * groups*n_cand entries of room. */
int64_t rqsid_match_workspace_bytes(int32_t groups);
int rqsid_match_to_candidates(const uint8_t* match, int32_t groups, int32_t n_cand,
                              int32_t* cand_base, int32_t* cand_count, int32_t* cand_idx,
                              uint8_t* seg_flags, void* workspace, int64_t workspace_bytes,
                              void* stream);

/* Dense distance matrix out[n][k] = sqrt(max(|x|^2 + |c|^2 - 2 x.c, 0)) in fp32
 * (torch.cdist semantics, pairwise_distance_full balancekmeans/__init__.py:576-603),
 * feeding the balanced auction. */
int rqsid_pairwise_distance(const float* x, int64_t n, int32_t dim, const float* centers,
                            int32_t k, float* out, void* stream);

/* Cosine distances 1 - x.c / (|x| |c|) of pairwise_cosine (balancekmeans/__init__.py:625-655, the
 * distance='cosine' option of KMeans.fit / fit_by_min_loss / predict, :279-280, 511-512): fp32 [n][k] into
 * `out` and / or the auction's worker-major fp16 scores -distance [k][n] into `out_wj` (either may be NULL).
 * fp32 sums in the kernel's order (the reference normalises the operands first, then multiplies: the
 * results agree to a few fp32 ulps of 1). */
int rqsid_pairwise_cosine(const float* x, int64_t n, int32_t dim, const float* centers, int32_t k, float* out,
                          uint16_t* out_wj, void* stream);

/* Auction score matrix: out_wj[k][n] = fp16(-||x_i - c_j||) (fp32 distances, half = 0) or
 * -max(fp16 distance of the fp16-rounded operands, 1e-5) (half != 0), worker-major: the input of
 * auction_lap_half(-pairwise_distance_{full,half}(X, C)), balancekmeans/__init__.py:29-43,
 * 536-603. */
int rqsid_auction_scores(const float* x, int64_t n, int32_t dim, const float* centers, int32_t k,
                         int32_t half, uint16_t* out_wj, void* stream);

/* Balanced assignment: the auction of balancekmeans.auction_lap_half (balancekmeans/__init__.py:
 * 12-140, return_token_to_worker=True) on the fp16 score matrix scores_wj[K][N] (worker-major,
 * IEEE half bits).  out_assign[j] = worker of job j.  Every fp16 operation of the reference is
 * reproduced with one rounding; ties at the top-k boundary keep the lowest job index and equal
 * highest bids go to the lowest worker (the reference leaves both to torch).  N < K reproduces
 * the reference's argmin(-D) fallback.  Blocks the calling thread (one host read per round);
 * *out_rounds = rounds run.  max_rounds <= 0: unbounded (the reference's leftover rule ends every
 * auction by round 1002). */
int64_t rqsid_auction_workspace_bytes(int64_t n_jobs, int32_t n_workers);
int rqsid_auction_lap_half(const uint16_t* scores_wj, int32_t n_workers, int64_t n_jobs,
                           int32_t max_rounds, int32_t* out_assign, int32_t* out_rounds,
                           void* workspace, int64_t workspace_bytes, void* stream);

/* The fp32 auction of balancekmeans.auction_lap_full (balancekmeans/__init__.py:142-210), reached only
 * through KMeans.predict(balanced=True) (:523-525), on fp32 scores scores_wj[K][N] (worker-major).
 * Every fp32 operation of the reference with one rounding; the same tie rules as rqsid_auction_lap_half.
 * Unlike auction_lap_half it has no N < K fallback: with jobs_per_worker = 0 nothing bids until the
 * leftover rule gives every job to worker 0 after round 1000.  Blocks the calling thread (one host read
 * per round); *out_rounds = rounds run.  N >= 1, 2 <= K <= 65535. */
int64_t rqsid_auction_full_workspace_bytes(int64_t n_jobs, int32_t n_workers);
int rqsid_auction_lap_full(const float* scores_wj, int32_t n_workers, int64_t n_jobs, int32_t max_rounds,
                           int32_t* out_assign, int32_t* out_rounds, void* workspace, int64_t workspace_bytes,
                           void* stream);

/* Segmented auction scores for many independent balanced fits at once (the per-parent sub-K-Means of
 * hierarchical_rq_kmeans.py:671-752 and the per-group sub-K-Means of :968-1053, which the reference runs
 * one after another, each through balancekmeans/__init__.py:29-43,536-603).  Segment s owns rows
 * seg_off[s] .. seg_off[s+1] of x (rows grouped by segment) and centres s*k .. s*k+k-1; its scores go to
 * out_wj + k*seg_off[s] as a [k][n_s] worker-major block, each value equal to rqsid_auction_scores on the
 * segment alone.  seg_tile_off[S+1] = exclusive scan of ceil(n_s / 64); n_tiles = seg_tile_off[S]. */
int rqsid_seg_auction_scores(const float* x, int64_t n, int32_t dim, const float* centers, int32_t k,
                             int32_t n_seg, const int32_t* seg_off, const int32_t* seg_tile_off,
                             int64_t n_tiles, int32_t half, uint16_t* out_wj, void* stream);

/* Segmented balanced assignment: one auction_lap_half (balancekmeans/__init__.py:12-140) per segment, all
 * segments advanced in lockstep (one launch sequence per round for all of them; a segment stops at its own
 * round count).  Segment s: jobs seg_off[s] .. seg_off[s+1] (n_s), scores at scores + k*seg_off[s] as
 * [k][n_s] fp16 (the layout of rqsid_seg_auction_scores).  Jobs are cut into chunks of
 * rqsid_seg_auction_chunk_jobs() that never straddle segments: seg_chunk_off[S+1] = exclusive scan of
 * ceil(n_s / chunk), total_chunks = seg_chunk_off[S]; n_multi = number of segments of more than one chunk
 * (checked).  active[s] (NULL = all) == 0 skips a segment (its out_assign entries are untouched).
 * out_assign[j] = worker of job j inside its segment; out_rounds[s] (device) = rounds run (0 for the
 * n_s < k fallback, argmin(-D) = the farthest centre, as the reference).  Each segment's result is
 * bit-identical to rqsid_auction_lap_half on its block alone.  Blocks the calling thread (one host read per
 * 8 rounds).  max_rounds <= 0: unbounded. */
int32_t rqsid_seg_auction_chunk_jobs(void);
int64_t rqsid_seg_auction_workspace_bytes(int64_t n_jobs, int32_t n_workers, int32_t n_seg,
                                          int64_t total_chunks, int32_t n_multi);
int rqsid_seg_auction_lap_half(const uint16_t* scores, int32_t n_workers, int32_t n_seg,
                               const int32_t* seg_off, const int32_t* seg_chunk_off, int64_t total_chunks,
                               int32_t n_multi, int64_t n_jobs, const uint8_t* active, int32_t max_rounds,
                               int32_t* out_assign, int32_t* out_rounds, void* workspace,
                               int64_t workspace_bytes, void* stream);

/* Row-sharded balanced assignment, one pass per call: the auction_lap_half of balancekmeans/__init__.py:
 * 12-140 over jobs spread across ranks (rank r owns a contiguous block of n_local of the n_global jobs,
 * scores [k][n_local] fp16 worker-major).  The caller (distributed.ShardedAuction) runs, per round,
 * hist(0) -> sum the [k][256] u32 histograms over ranks -> select(0) -> hist(1) -> sum -> select(1) ->
 * eqcount -> rank_off[w] = eqtot[w] summed over lower ranks -> bid(rank_off) -> resolve -> sum `have`
 * over ranks -> end_round, and stops when the summed `have` equals n_global; after begin it reduces the
 * {max, min} order keys (max / min over ranks) and calls eps.  Every fp16 operation and the tie rule
 * (lowest GLOBAL job index at the top-k boundary, lowest worker among equal bids) are those of
 * rqsid_auction_lap_half, so the assignment equals the single-process auction of the whole matrix.
 * rqsid_dauction_layout gives the byte offsets, inside the workspace, of the buffers the caller
 * reduces: [0] u32[2] {max key, min key} (min initialised to 0xFFFFFFFF), [1] u32 [k][256] histogram
 * followed by one u32 (summed with it: the ranks whose bid list overflowed), [2] u32 [k] eqtot, [3] u32
 * have, and the state it may poll: [4] u8 flag (bit 0: still bidding; cleared by rqsid_dauction_end_round
 * once the reduced `have` equals n_global, after which every pass is a no-op, so the caller need not read
 * it every round), [5] i32 rounds run.  `offsets` holds 6 entries.
 * Bid lists (RQSID_DAUCTION_LIST=0 turns them off): from round 32 (16 at k >= 1024) a round slot may run
 * from per-rank lists of each worker's values near its threshold instead of sweeping the scores, with the
 * same calls and collectives in the same order (the histograms then count listed values).  When the
 * reduced data show a list did not hold, the slot is void (no job state changes, the round does not
 * count) and the next slot runs that round as a sweep; the result is the sweep's in every case. */
int64_t rqsid_dauction_workspace_bytes(int64_t n_local, int32_t n_workers);
/* List-only round slots: workspace bytes [192, 196) hold the mode of the coming slot (u32: 0 sweep, 1 list,
 * 2 void), identical on every rank.  While it reads 1 the caller may run a slot as list_pass(-1),
 * list_pass(0), sum, select(0), list_pass(1), sum, select(1), list_pass(2), gather, list_pass(3, rank_off),
 * resolve, sum, end_round: the same collectives without launching the sweep kernels; a list-only slot that
 * meets a sweep round is void (nothing changes) and the caller returns to full slots at its next poll. */
/* Diagnostics of the row-sharded list state: out (device u32[8]) = {coming slot's mode, round, longest list,
 * mean list length, worker 0's list base key, worker 0's threshold key, summed overflow word, lists over
 * capacity}. */
int rqsid_dauction_debug(const uint16_t* scores, int32_t n_workers, int64_t n_local, int64_t n_global, uint32_t* out,
                         void* workspace, int64_t workspace_bytes, void* stream);
int rqsid_dauction_list_pass(const uint16_t* scores, int32_t n_workers, int64_t n_local, int64_t n_global,
                             int32_t step, const uint32_t* rank_off, void* workspace, int64_t workspace_bytes,
                             void* stream);
int rqsid_dauction_layout(int64_t n_local, int32_t n_workers, int64_t* offsets);
int rqsid_dauction_begin(const uint16_t* scores, int32_t n_workers, int64_t n_local, int64_t n_global,
                         int32_t* out_assign, void* workspace, int64_t workspace_bytes, void* stream);
int rqsid_dauction_eps(const uint16_t* scores, int32_t n_workers, int64_t n_local, int64_t n_global,
                       void* workspace, int64_t workspace_bytes, void* stream);
int rqsid_dauction_hist(const uint16_t* scores, int32_t n_workers, int64_t n_local, int64_t n_global,
                        int32_t low, void* workspace, int64_t workspace_bytes, void* stream);
int rqsid_dauction_select(const uint16_t* scores, int32_t n_workers, int64_t n_local, int64_t n_global,
                          int32_t low, void* workspace, int64_t workspace_bytes, void* stream);
int rqsid_dauction_eqcount(const uint16_t* scores, int32_t n_workers, int64_t n_local, int64_t n_global,
                           void* workspace, int64_t workspace_bytes, void* stream);
int rqsid_dauction_bid(const uint16_t* scores, int32_t n_workers, int64_t n_local, int64_t n_global,
                       const uint32_t* rank_off, void* workspace, int64_t workspace_bytes, void* stream);
int rqsid_dauction_resolve(const uint16_t* scores, int32_t n_workers, int64_t n_local, int64_t n_global,
                           int32_t* out_assign, void* workspace, int64_t workspace_bytes, void* stream);
int rqsid_dauction_end_round(const uint16_t* scores, int32_t n_workers, int64_t n_local, int64_t n_global,
                             void* workspace, int64_t workspace_bytes, void* stream);

/* Greedy unique-nearest match rows (_assign_last_match_matrix hierarchical_rq_kmeans.py:1022-1038,
 * _get_dynamic_match_matrix simplified_semantic_id_generator.py:282-291): group g owns rows
 * sub_off[g]..sub_off[g+1] of dist [total][n_cand]; its first min(rows, max_take) rows each take, in
 * order, their nearest still-unused column (lowest column on exact ties).  match [groups][n_cand]
 * gets 1 for taken columns, n_selected[g] their count (the reference's random fill is host work). */
int rqsid_greedy_match(const float* dist, const int32_t* sub_off, int32_t groups, int32_t n_cand,
                       int32_t max_take, uint8_t* match, int32_t* n_selected, void* stream);

/* Numerics probe (self-test): d = a.b + c with ONE v_mfma_f32_32x32x16_f16 (f16 == 1) or
 * _bf16 (f16 == 0); a [32][16], b [16][32] (half / bfloat16 bits), c/d fp32 [32][32], row-major.  The tests
 * use it to pin the MFMA accumulation model behind rqsid_assign's screening bound.  f16 == 2: ONE
 * v_mfma_scale_f32_32x32x64_f8f6f4 on OCP fp8 e4m3 bytes with unit scales, a [32][64], b [64][32] (the
 * pointers then address bytes). */
int rqsid_mfma_probe(int32_t f16, const uint16_t* a, const uint16_t* b, const float* c, float* d,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RQSID_H */
