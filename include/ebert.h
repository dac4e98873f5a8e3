/*
 * ebert.h -- C ABI of the MI355X-native embedding-similarity retrieval engine (libebert.so).
 *
 * This is the drop-in boundary for the reference's recommend/top-K hot path:
 *   /root/reference/src/backend/app/lib.py:51-55   cosine_similarity -> mean -> exclude rated
 *                                                   -> sort_values(desc)[:k]
 *   /root/reference/src/backend/app/lib.py:105-106  the same mean-cosine for search re-weighting
 *   /root/reference/src/backend/app/constants.py:55-56  catalog residency (load-time)
 * The reference has no plugin/operator API for this path; the seam is that inline block, so the
 * entry points below are what its Python binding (ctypes) calls in place of
 * scikit-learn `cosine_similarity` (metrics/pairwise.py:1683-1738) and the pandas sort.
 *
 * Conventions
 *   - Every pointer argument is DEVICE memory owned by the caller (torch tensors), except where
 *     a comment says "host". The library never allocates or frees caller memory; scratch space
 *     is a caller-provided workspace sized by ebt_cosine_topk_workspace().
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream). Every entry point only
 *     enqueues work on that stream and returns; nothing synchronises except ebt_timer_query().
 *   - Return value: EBT_OK (0) or a negative EBT_E* code; the message of the last failure on the
 *     calling thread is available from ebt_last_error(). All entry points are reentrant: no
 *     mutable global state apart from the thread-local error string and a per-device cache of
 *     the compute-unit count (atomic; every writer stores the same value).
 *   - Row ids: catalog rows are addressed by their row number inside the (shard-local) matrix;
 *     results carry GLOBAL row ids = local row + row_offset (a catalog row-sharded over ranks).
 *   - Ordering of every top-k result: score descending, then row ascending. The reference's
 *     pandas sort is an unstable introsort (pandas core/sorting.py:436-441), so its tie order is
 *     unspecified; this is the deterministic order the build defines.
 *   - Non-finite catalog rows: a row holding a NaN or an infinity has a NaN cosine against every
 *     query; such a row is never a candidate on any path (the selects, merges, the filter
 *     epilogue and the large-k sort all drop NaN scores), so it only shows as an empty NaN / -1
 *     slot when k exceeds the remaining candidates. pandas would list it last with score NaN
 *     (sort_values(na_position="last")); the reference's catalogs are finite ALS / embedding
 *     factors, and no reference fixture holds a non-finite row (parity unpinned on this edge).
 */
#ifndef EBERT_H_
#define EBERT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---------------------------------------------------------------------- */
#define EBT_OK 0
#define EBT_EINVAL (-1)      /* bad argument (shape, dtype, null pointer, k/kprime range)   */
#define EBT_EHIP (-2)        /* a HIP runtime call or kernel launch failed                    */
#define EBT_ENOMEM (-3)      /* workspace too small                                           */
#define EBT_EUNSUPPORTED (-4)

/* ---- element types --------------------------------------------------------------------- */
#define EBT_F32 0
#define EBT_BF16 1
#define EBT_F16 2
#define EBT_F64 3

/* Library version (major*10000 + minor*100 + patch).
 * 0.2.0: ebt_rescore gained `timer`; ebt_comm gained the trailing `all_reduce_f64` pointer (the
 *        library calls it whenever it is non-NULL: zero-initialise every ebt_comm).
 * 0.3.0: ebt_timer_count_rows / ebt_timer_rows (additive).
 * 0.3.1: eps from the measured image errors (ebt_query_image); ebt_catalog_init measures u_cat
 *        and its state holds 256 bytes more for a non-native catalog (ebt_catalog_state_bytes);
 *        ebt_cosine_sample_lead / ebt_cosine_screen_at_lead (additive).
 * 0.3.2: ebt_sort_exclusions and the full-sort path hand-written (workspace sizes shrink; host
 *        arithmetic only); the exclusion-order check of ebt_cosine_topk* runs inside the rescore
 *        (certified = -3 from ebt_cosine_topk_prepared / ebt_rescore's callers for a query whose
 *        segment is not ascending); ebt_shard_sample_tiles (additive); the row counter of
 *        ebt_timer_count_rows is device-aware.
 * 0.3.3: a pinned certificate buffer of ebt_cosine_topk_submit / ebt_cosine_topk_sharded_submit
 *        is written by the kernels themselves (no copy launch; EBT_EHIP from _finish if one was
 *        not delivered); the speculative screen's segment thresholds come from its wave merges;
 *        ebt_merge_packed also flags a query with more than min(R k, 2 k + 256) entries.
 * 0.4.0: live catalog updates: ebt_catalog_init_reserved, ebt_catalog_update_bytes,
 *        ebt_catalog_update_rows, ebt_catalog_append_rows (additive; struct ebt_catalog and
 *        ebt_catalog_init are unchanged).
 * 0.5.0: rows removed in place: ebt_catalog_remove_bytes, ebt_catalog_remove_plan,
 *        ebt_catalog_remove_rows (additive).
 * 0.6.0: per-query allow masks: ebt_allow, ebt_allow_words, ebt_allow_from_bool,
 *        ebt_allow_set_rows, ebt_mask_allowed, ebt_cosine_topk_prepared_allowed,
 *        ebt_cosine_topk_allowed / _allowed_submit / _allowed_finish (additive; no existing
 *        struct or signature changes; ebt_workspace_bytes grows by the retry group's mask ids,
 *        at most 1 KiB).
 * 0.7.0: materialised sub-catalogs: ebt_allow_count, ebt_allow_rows_bytes, ebt_allow_rows,
 *        ebt_catalog_gather_rows, ebt_sub_exclusions_bytes, ebt_sub_exclusions,
 *        ebt_sub_rows_to_global (additive; no existing entry, struct or kernel changes).
 * 0.8.0: per-row weights on liked-row queries: ebt_query_liked_wsum, ebt_cosine_topk_weighted /
 *        _weighted_submit, ebt_cosine_topk_sharded_weighted / _sharded_weighted_submit
 *        (additive; liked_w == NULL launches the kernels of 0.7.0; no workspace size changes).
 * 0.9.0: explanations, the per-liked-row terms of a returned score: ebt_explain_workspace_bytes,
 *        ebt_liked_contrib, ebt_explain_select, ebt_explain_topk (additive; no existing kernel,
 *        struct, signature or workspace size changes).
 * 0.10.0: diversified top-k, greedy maximal marginal relevance over a candidate pool:
 *        ebt_mmr_workspace_bytes, ebt_pool_gram, ebt_mmr_select, ebt_mmr_topk (additive; no
 *        existing entry, struct, kernel or workspace size changes).
 * 0.11.0: multi-interest top-k, cluster the liked rows and interleave the per-cluster answers:
 *        ebt_interest_workspace_bytes, ebt_interest_cluster, ebt_liked_interests,
 *        ebt_interest_interleave (additive; no existing entry, struct, kernel or workspace size
 *        changes).
 * 0.12.0: grouped top-k, one list per (query, group) from one scoring pass:
 *        ebt_grouped_pass_groups, ebt_select_topk_grouped, ebt_cosine_topk_grouped_workspace,
 *        ebt_cosine_topk_grouped_prepared (additive; no existing entry, struct, kernel or
 *        workspace size changes). */
int ebt_version(void);

/* Message for the last non-zero return on this thread ("" if none). */
const char* ebt_last_error(void);

/* ---- catalog load: constants.py:55-56 (+ sklearn row_norms, preprocessing/_data.py:2011) ---
 * Guarded L2 norm of every row in float64: gnorm[i] = ||x_i|| unless ||x_i|| < 10*DBL_EPSILON,
 * in which case 1.0 (sklearn _handle_zeros_in_scale, preprocessing/_data.py:118-123), and the
 * float32 reciprocal inv32[i] = 1/gnorm[i] used by the screening epilogue. inv32 may be NULL.
 * x: n rows of d elements of `dtype`, row stride `ld` ELEMENTS. */
int ebt_row_norms(const void* x, int dtype, int64_t n, int32_t d, int64_t ld,
                  double* gnorm64, float* inv32, void* stream);

/* Screening image of a matrix: img[i][j] = round_to(img_dtype, x[i][j] * s_i) for j < d and 0 for
 * d <= j < ld_img, where s_i = 1/gnorm64[i] if `normalize` else 1. img_dtype is EBT_F16 or
 * EBT_BF16; ld_img (row stride in elements) must be a multiple of 64 and >= d. Rows of the
 * image past n are not touched. */
int ebt_screen_image(const void* x, int dtype, int64_t n, int32_t d, int64_t ld,
                     const double* gnorm64, int normalize, int img_dtype, void* img,
                     int32_t ld_img, void* stream);

/* ---- queries: lib.py:51-52 folded into one query vector per user -------------------------
 * Dense queries (one vector per query, the L = 1 case of lib.py:51):
 *   q64[b] = q[b] / gnorm(q[b])  (float64, sklearn normalize semantics).
 * Liked-rows queries (the collaborative path): for CSR lists liked_off[B+1] / liked_rows[] of
 * LOCAL catalog rows, q64[b] = sum_l cat[l] / gnorm64_cat[l]  (a SUM; the caller divides by the
 * user's liked count L_b after an optional cross-shard all-reduce). liked_off/liked_rows NULL
 * selects the dense form. q64 is B x d float64, row stride d. */
int ebt_query_dense(const void* q, int dtype, int64_t B, int32_t d, int64_t ldq, double* q64,
                    void* stream);
int ebt_query_liked_sum(const void* cat, int dtype, int32_t d, int64_t ld,
                        const double* gnorm64_cat, int64_t B, const int64_t* liked_off,
                        const int64_t* liked_rows, double* q64, void* stream);
/* ebt_query_dense + ebt_query_image in one launch for dense queries (d <= 4096; same q64,
 * qimg, qscale and eps; with native_q the query dtype must equal img_dtype). */
int ebt_query_prep(const void* q, int dtype, int64_t B, int64_t B_pad, int32_t d, int64_t ldq,
                   int img_dtype, int native_q, float u_cat, double* q64, void* qimg,
                   int32_t ld_img, float* qscale, float* eps, void* stream);
/* q64[b] *= scale[b] (scale is device float64[B]); used for the 1/L of lib.py:52. */
int ebt_scale_rows_f64(double* q64, int64_t B, int32_t d, const double* scale, void* stream);

/* Screening image + certification bound of a query batch.
 *   qimg[b][j] = round_to(img_dtype, q64[b][j]) (rows B..B_pad-1 and columns d..ld_img-1 = 0),
 *   qscale[b]  = 1,
 *   eps[b]     = a rigorous bound on |approx score - exact float64 score| for every catalog
 *                row, given `u_cat` >= ||image row - row/gnorm||_2 for every row (0 for a
 *                native image whose values are exact; ebt_catalog_init measures it for a
 *                float16-rounded normalised image, and the unit round-off 2^-11 always holds):
 *                eps = 1.05*(dq + |q|*u_cat + dq*u_cat + (d+8)*2^-24*(|q|+1)) + 1e-9,
 *                with dq = ||qimg[b] - q64[b]||_2 measured by the kernel (ABI 0.3.1; before it
 *                dq was bounded by |q| times the unit round-off of img_dtype).
 * With `native_q` != 0 the image is instead the raw query `q` (same dtype as img_dtype, the
 * native-catalog screening mode): qimg = q, qscale[b] = 1/gnorm(q[b]) and dq = 0. */
int ebt_query_image(const double* q64, int64_t B, int64_t B_pad, int32_t d, int img_dtype,
                    const void* q_native, int64_t ldq, int native_q, float u_cat, void* qimg,
                    int32_t ld_img, float* qscale, float* eps, void* stream);

/* ---- kernels of the search pipeline (exposed for tests and the bench) --------------------
 * Screening GEMM on MFMA: scores[b][i] = qscale[b]*cscale[i]*sum_j qimg[b][j]*cimg[i][j] for
 * b < B_pad (multiple of 128) and i < n_rows; f16 or bf16 inputs, float32 accumulate.
 * cscale may be NULL (= 1). ld_scores must be a multiple of 4 and >= n_rows. */
int ebt_screen_scores(const void* qimg, int64_t B_pad, const void* cimg, int64_t n_rows,
                      int32_t d_pad, int32_t ld_img, int img_dtype, const float* qscale,
                      const float* cscale, float* scores, int64_t ld_scores, void* stream);

/* The fused screen's GEMM: the same product, but only scores >= thr[b] leave the kernel.
 * Catalog rows are grouped by G = ebt_filter_group_rows(B_pad) (the kernel's tile: 256 rows
 * when B_pad % 256 == 0, else 128); the first `slots` hits of query b in group g go to
 * cand[b*ld_cand + g*slots + p] as u64 composites (order-preserving key of the f32 score << 32 |
 * ~(uint32)(idx_base + local row)), and counts[b*ld_counts + g] = the group's hit count
 * (saturated at 255). A count above `slots` drops hits and sets ovf[b] = 1. Buffers have B_pad
 * rows, 1 <= slots <= EBT_FILTER_SLOTS_MAX, ld_cand >= groups*slots, ld_counts >= groups; thr
 * has B_pad entries (+inf for padding). */
#define EBT_FILTER_SLOTS_MAX 128
int64_t ebt_filter_group_rows(int64_t B_pad);
/* Long filter launches (0.3.0): a fused segment of the pipeline (ebt_cosine_topk*, ebt_cosine_screen*)
 * over more than ~1.5 x T x (CUs / query tiles) tiles of 256 rows is run as consecutive
 * ebt_screen_filter launches of whole rounds, each at most T tiles per workgroup
 * (default T = 32 since 0.3.1, 512 in 0.3.0; EBT_FILTER_TPW in the environment), so that the persistent walk's
 * workgroups start in step again (screening GEMM). Same tiles, hits and counts.
 * ebt_filter_split(T) sets T for the process (0: never split; T < 0: query) and returns the
 * previous value. */
int64_t ebt_filter_split(int64_t tiles_per_workgroup);
int ebt_screen_filter(const void* qimg, int64_t B_pad, const void* cimg, int64_t n_rows,
                      int32_t d_pad, int32_t ld_img, int img_dtype, const float* qscale,
                      const float* cscale, const float* thr, uint64_t* cand, int64_t ld_cand,
                      int32_t slots, uint8_t* counts, int64_t ld_counts, int32_t* ovf,
                      int64_t idx_base, void* stream);

/* Excluded rows (lib.py:48,55: rated movies are not candidates): for every b < B and every
 * GLOBAL row g in excl_rows[excl_off[b] .. excl_off[b+1]) with col_begin <= g < col_end,
 * scores[b][g - col_begin] = -inf. */
int ebt_mask_excluded(float* scores, int64_t ld_scores, int64_t B, int64_t col_begin,
                      int64_t col_end, const int64_t* excl_off, const int64_t* excl_rows,
                      void* stream);

/* Streaming top-k' select (one HBM pass over the scores): for each row b < B and each of `segs`
 * equal segments of its n entries, write the kprime largest (value desc, index asc) entries,
 * sorted, to out_vals/out_idx[b*ld_out + seg*kprime + j]. Entries that are NaN or -inf are
 * never selected; missing slots get -inf / -1. Dense form (idx == NULL): the index of entry j
 * is idx_base + j. Candidate-list form: idx[b*ld + j] gives it (values < 2^31, -1 = empty).
 * 1 <= kprime <= 4096. */
int ebt_select_topk(const float* vals, const int64_t* idx, int64_t ld, int64_t B, int64_t n,
                    int64_t idx_base, int32_t kprime, int32_t segs, float* out_vals,
                    int64_t* out_idx, int64_t ld_out, void* stream);

/* Exact float64 rescore of the screened candidates + final top-k + certification.
 * For each b: candidates cand_rows[b*kprime + j] (LOCAL rows, -1 = empty), sorted by their
 * approx scores cand_vals (desc). score = (q64[b] . cat[row]) / gnorm64[row] in float64; the k
 * best by (score desc, row asc) go to out_scores/out_rows[b*k + j] (rows + row_offset; empty
 * slots NaN / -1). certified[b] = 1 iff the candidate set provably contains the exact top-k:
 * kprime >= n_rows (every row is a candidate),
 * fewer than kprime valid candidates, or approx[kprime-1] < cut[b] (below, after its rise).
 * n_rows is the catalog's row count; a candidate row >= n_rows is never read and gives
 * certified[b] = -2 (corrupt candidate list).
 * Candidates with approx < cut[b] = max(approx[k-1] - 2*eps[b], t_floor[b] - eps[b]) cannot
 * be in the top k and are not gathered (equal cand_vals and eps = 0 rescore every candidate).
 * With eps[b] > 0 the cut then rises to s_min - eps[b], s_min = the smallest exact score of the
 * list's first k entries (k rows score >= s_min, so a row with exact < s_min is not in the top
 * k): those k are scored first and later candidates below the raised cut are skipped. t_floor
 * (float64 [B], NULL = none) is a lower bound of the k-th best EXACT score over the whole
 * (sharded) catalog, e.g. the all-reduced max over shards of approx[k-1] - eps: a shard then
 * rescores only rows that can enter the GLOBAL top k, and the slots of its top k that such a
 * cut leaves empty read NaN / -1: the certificate is then about the GLOBAL top k (a row
 * dropped below approx[kprime-1] < t_floor - eps has exact < t_floor). */
int ebt_rescore(const double* q64, int64_t B, int32_t d, const void* cat, int dtype, int64_t ld,
                const double* gnorm64, int64_t row_offset, const float* cand_vals,
                const int64_t* cand_rows, int32_t kprime, int32_t k, int64_t n_rows, const float* eps,
                const double* t_floor, double* out_scores, int64_t* out_rows, int32_t* certified,
                void* timer, void* stream);

/* Diagnostics of the rescore's arithmetic (tests, A/B tools; not needed by a caller).
 * ebt_rescore_form(form): which form of the exact dot products ebt_rescore (and every entry
 * point that rescores) launches from now on, process-wide: 1 = the lane's query values held in
 * registers (the default where d fits 512 16-byte chunks), 0 = the query staged in LDS; -1
 * leaves it. Returns the form in effect before the call. Both forms give bitwise equal scores.
 * ebt_wave_sum_check: for each of n_waves waves of 64 doubles in[64 w + l], out_a[64 w + l] =
 * the library's wave sum (cross-lane VALU moves), out_b[...] = the same xor butterfly through
 * shuffles; the two are expected bitwise equal in every lane. */
int ebt_rescore_form(int form);
int ebt_wave_sum_check(const double* in, int64_t n_waves, double* out_a, double* out_b,
                       void* stream);

/* The fused screen's merge step: query b's candidate list (fv/fi[b*kprime + j], a PARTITIONED
 * list: see below; a sorted list, as ebt_select_topk leaves it, is one) and the hits
 * ebt_screen_filter left in `n_groups` groups of cand/counts (same slots/ld as that call) -> the
 * kprime best of both, back into fv/fi, partitioned at k (1 <= k <= kprime):
 *   [0, k-1) the k-1 best in any order, [k-1] the k-th best, [k, n-1) the rest in any order,
 *   [n-1] the smallest kept, [n, kprime) empty (-inf / -1), n = min(kprime, entries).
 * (Lists of k' > 512, merged by the block kernel, come back fully sorted: also partitioned.)
 * Exclusions (GLOBAL rows, CSR sorted per query, or NULL) are dropped from the hits; a group
 * count above `slots`, or more hits than the merge holds, sets ovf[b] = 1. */
int ebt_merge_hits(float* fv, int64_t* fi, int64_t B, int32_t kprime, int32_t k,
                   const uint64_t* cand, int64_t ld_cand, int32_t slots, const uint8_t* counts,
                   int64_t ld_counts, int64_t n_groups, int64_t row_offset,
                   const int64_t* excl_off, const int64_t* excl_rows, int32_t* ovf, void* stream);
/* Groups one block merge (k' > 512) indexes at once: its LDS holds the list + hit entries and a
 * u16 position per group; ebt_merge_hits merges more groups in consecutive parts of this many
 * (rounded down to 16). Host call, no device work after the first (reads the kernel's static
 * LDS size). */
int64_t ebt_merge_block_max_groups(int32_t kprime);

/* Exclusion CSR order: the search entry points binary-search each exclusion segment and take
 * it sorted ascending. ebt_sort_exclusions sorts every segment of a caller's CSR on the device:
 * segment b = rows_in[off[b] .. off[b+1]) (ABSOLUTE positions, off[0] may be > 0), sorted into
 * the same positions of rows_out; positions outside every segment are copied unchanged; rows_out
 * may equal rows_in. nnz = the length of the rows array. Offsets are clamped into [0, nnz] before
 * use (a malformed CSR is then rejected by the search entry's own check). Workspace: device,
 * ebt_sort_exclusions_bytes(B, nnz) bytes (0 = invalid sizes: B < 1 or > 2^24, nnz >= 2^31;
 * 0.3.2: one hand-written launch, 8 * nnz bytes of workspace). */
size_t ebt_sort_exclusions_bytes(int64_t B, int64_t nnz);
int ebt_sort_exclusions(const int64_t* off, const int64_t* rows_in, int64_t* rows_out, int64_t B,
                        int64_t nnz, void* workspace, size_t ws_bytes, void* stream);

/* Merge R partial top-k lists (scores/rows [R][B][k], each sorted) into the global top-k per
 * query -- the post-all-gather step of a row-sharded catalog. k <= 4096, any R. */
int ebt_merge_topk(const double* scores, const int64_t* rows, int32_t R, int64_t B, int32_t k,
                   double* out_scores, int64_t* out_rows, void* stream);

/* The compact form of that exchange (what the row-sharded step sends). After the catalog-wide
 * floor (ebt_union_floor), a shard's entries below t_floor[b] -- a lower bound of query b's k-th
 * best exact score over the WHOLE catalog -- cannot enter the global top k. ebt_shard_pack keeps
 * of each sorted list (scores/rows [B][k], row < 0 = padding; t_floor NULL = keep every real
 * entry) the prefix with score >= t_floor[b] and packs it into `send`
 * (ebt_shard_pack_bytes(B, cap) bytes, device): u32 start[B], u32 len[B] (query b's entries are
 * [start[b], start[b] + len[b]); 0.3.2 -- the starts are prefix sums of the lengths in query
 * order, from ebt_shard_pack or, in the sharded C entry, from the lengths its rescore wrote)
 * and block totals, then f64 scores[cap], then i32 GLOBAL rows[cap]. Entries at positions
 * >= cap are counted but not sent. After an all-gather of the R buffers
 * (recv, R * ebt_shard_pack_bytes bytes, rank order), ebt_merge_packed writes the same global
 * top-k as ebt_merge_topk over the full lists, and sets *incomplete (device int32; set to 1,
 * never cleared) when some rank's entries did not all fit its cap, or (0.3.3) when one query
 * received more than min(R k, 2 k + 256) entries (a floor band wider than k + 256): the caller
 * must then merge the full lists instead (the rows of an incomplete batch are not final).
 * ebt_shard_pack_cap: the cap the library uses, B * ebt_shard_list_width(k, world), or 0 when
 * the compact form does not apply (world < 2, world * k > 8192, n_global >= 2^31).
 * ebt_shard_list_width(k, world) = min(k, ceil(1.5 k / world) + 8): also the per-shard width of
 * the floor all-gather (a shard's widest share of the global top k, with margin; a narrower
 * floor is still a valid lower bound). */
int64_t ebt_shard_list_width(int32_t k, int32_t world);
/* The shared screening threshold's sample of the row-sharded step (0.3.2, host arithmetic): the
 * 256-row tiles each shard samples for this catalog size, world and padded batch (0 = every
 * shard screens at its own threshold; -1 bad arguments). The same rule as distributed.py
 * shared_sample_tiles; world * 4 * tiles <= 2048 (ebt_pool_kth's limit). */
int64_t ebt_shard_sample_tiles(int64_t n_global, int32_t world, int64_t B_pad);
int64_t ebt_shard_pack_cap(int64_t B, int32_t k, int32_t world, int64_t n_global);
size_t ebt_shard_pack_bytes(int64_t B, int64_t cap);
int ebt_shard_pack(const double* scores, const int64_t* rows, int64_t B, int32_t k,
                   const double* t_floor, int64_t cap, void* send, void* stream);
int ebt_merge_packed(const void* recv, int32_t R, int64_t B, int32_t k, int64_t cap,
                     double* out_scores, int64_t* out_rows, int32_t* incomplete, void* stream);

/* Exact screen: scores[b*ld_scores + j] = (float)((q64_b . c_j) / gnorm64_j) in float64
 * arithmetic for every row j < n_rows (no replacement in the reference: the fallback screen of
 * EBT_FLAG_EXACT, whose only error is the final f32 rounding). */
int ebt_screen_exact(const double* q64, int64_t B, int32_t d, const void* cat, int dtype,
                     int64_t ld, const double* gnorm64, int64_t n_rows, float* scores,
                     int64_t ld_scores, void* stream);

/* ---- the whole pipeline -------------------------------------------------------------------
 * flags: EBT_FLAG_NO_FUSE disables the fused screen (every score row is materialised).
 * EBT_FLAG_EXACT screens with ebt_screen_exact instead of the MFMA image (unfused; qimg,
 * qscale, eps and cimg may be NULL): the last resort for a query that cannot be certified at
 * kprime = 4096, certified with eps = EBT_EXACT_EPS (|q64| <= 1 as the ebt_query_* make it). */
#define EBT_FLAG_NO_FUSE 1
#define EBT_FLAG_EXACT 2
#define EBT_FLAG_THETA 4 /* internal: set by ebt_cosine_screen_at (workspace sizing only) */
#define EBT_EXACT_EPS 1.1920928955078125e-07f /* 2^-23 >= f32 rounding of |s| <= 1 + f64 error */
/* How ebt_cosine_topk_prepared will run these sizes (host pointers out): head rows screened unfused,
 * the largest fused tail segment in rows (cap; 0 = not fused), score chunk rows, fused flag. */
int ebt_cosine_topk_plan(int64_t B, int64_t B_pad, int64_t n_rows, int32_t kprime,
                         int64_t chunk_rows, int flags, int64_t* head_rows, int64_t* cap,
                         int64_t* chunk, int32_t* fused);
/* The speculative fused screen ebt_cosine_topk_prepared uses for these sizes (all 0: not used).
 * sample_tiles full 256-row tiles, tile_stride tiles apart (tiles 0, s, 2s, ...), go through the
 * screening GEMM keeping only each query's max per 64-row subgroup; the rank-th largest of those
 * maxima is the query's speculative threshold theta for one filter pass over the whole catalog;
 * hits = the expected hits per query. theta is checked afterwards (theta <= the k-th best approx
 * - 2 eps, else certified = -1: rerun unfused), so it never costs exactness. */
int ebt_cosine_topk_spec_plan(int64_t B, int64_t B_pad, int64_t n_rows, int32_t kprime,
                              int flags, int64_t* sample_tiles, int64_t* tile_stride,
                              int32_t* rank, double* hits);
/* The speculative screen's lead (0.3.0): its sample's first `lead` tiles are the catalog's first
 * tiles (the rest of the sample strided after them: tiles 0 .. lead-1, lead, lead + s, ...), their
 * scores are kept and their hits taken at theta, and the filter GEMM covers rows [256 lead, n)
 * only -- lead is chosen so that those are whole rounds of the persistent grid (one 256 x 256
 * output tile per CU and round); every segment but the last is whole rounds too. Returns the
 * lead in tiles (0: none; -1: bad arguments). ebt_spec_lead(on) switches it on (1, default) or
 * off (0) for the process (on < 0: query); returns the previous setting. Results are the same
 * either way: the lead's hits are the filter's own, value for value. */
int64_t ebt_cosine_topk_spec_lead(int64_t B, int64_t B_pad, int64_t n_rows, int32_t kprime,
                                  int flags);
int ebt_spec_lead(int on);
/* Workspace bytes needed by ebt_cosine_topk_prepared for these sizes. */
size_t ebt_cosine_topk_workspace(int64_t B, int64_t B_pad, int64_t n_rows, int32_t kprime,
                                 int64_t chunk_rows, int flags);

/* The prepared-query pipeline under ebt_cosine_topk (one pass, no retries): query x catalog
 * cosine top-k over one (shard of a) catalog:
 *   unfused: for every catalog chunk of chunk_rows rows: screening GEMM -> mask excluded ->
 *   streaming select of kprime candidates; then a select across chunks; then the exact float64
 *   rescore.
 *   speculative fused (default for B_pad % 256 == 0, kprime <= 512 and >= 8 sample tiles, see
 *   ebt_cosine_topk_spec_plan): a pooled sample gives each query a threshold, the whole catalog
 *   is filtered in a few large segments (later ones at max(theta, the list's k-th - 2 eps)),
 *   then theta is verified (failure: certified = -1).
 *   fused (otherwise, when n_rows >= 2*H, H = max(65536, 256*kprime)): the head rows [0, H) go
 *   through the unfused path; the k'-th best head score of each query is a lower bound of its
 *   global k'-th best. The tail rows [H, n) are screened in doubling segments (each as large as
 *   all rows before it): the GEMM appends only scores >= the query's current bound to its
 *   candidate list (epilogue filter: no score matrix in HBM), exclusions are removed from the
 *   list (excl_rows must be sorted ascending per query), the k' best are kept and the bound is
 *   raised to their k'-th score before the next segment -- about k' appends per query per
 *   segment. The final k' are rescored. certified[b] = -1 reports a segment whose appends
 *   exceeded the capacity (rerun the query with EBT_FLAG_NO_FUSE).
 * Inputs: the query batch prepared by ebt_query_* (q64, qimg, qscale, eps; B real rows, B_pad
 * image rows), the catalog (cat/dtype/ld with gnorm64; its screening image cimg with cscale or
 * NULL, ld_img, d_pad), exclusions as CSR of GLOBAL rows (NULL = none), k <= kprime.
 * Outputs: out_scores (float64 [B][k]), out_rows (int64 [B][k], global), certified (int32 [B]);
 * certified[b] = -3 when query b's exclusion segment is not ascending (checked by the rescore,
 * 0.3.2: its results are then not valid). timer (NULL or an ebt_timer) collects per-stage GPU
 * time. */
int ebt_cosine_topk_prepared(const double* q64, const void* qimg, const float* qscale, const float* eps,
                    int64_t B, int64_t B_pad, const void* cat, int dtype, int64_t ld,
                    const double* gnorm64, const void* cimg, const float* cscale, int img_dtype,
                    int32_t ld_img, int64_t n_rows, int32_t d, int32_t d_pad, int64_t row_offset,
                    const int64_t* excl_off, const int64_t* excl_rows, int32_t k, int32_t kprime,
                    int64_t chunk_rows, int flags, void* workspace, size_t ws_bytes,
                    double* out_scores, int64_t* out_rows, int32_t* certified, void* timer,
                    void* stream);

/* ---- the self-contained path: one call per batch ------------------
 * What a non-Python caller binds (cgo / JNI / N-API / ctypes): raw queries
 * in, certified float64 top-k out; query prep, the screen, the certificate check and every
 * retry (fused-list overflow -> unfused rerun, uncertified -> k' x 4 -> float64 screen) run
 * inside the library. Replaces /root/reference/src/backend/app/lib.py:51-55 (cosine_similarity
 * of the liked rows against the catalog, mean over them, exclusion of rated rows, descending
 * sort, [:k]) for a batch of users, and constants.py:55-56 (the resident catalog).
 *
 * ebt_catalog: the resident (shard of a) catalog, filled by ebt_catalog_init from the caller's
 * device matrix and a caller-provided device STATE buffer of ebt_catalog_state_bytes() bytes
 * (float64 guarded row norms, float32 inverse norms, and the f16 screening image unless the
 * matrix itself is the MFMA operand: f16 / bf16 with d, ld % 64 == 0). Afterwards it changes
 * only through the live-update entries below (0.4.0, 0.5.0), which rewrite rows and their state in place;
 * the struct and the state buffer must outlive every call that uses them. For a non-native
 * catalog (f32 / f64) ebt_catalog_init waits for `stream` once, to read back u_cat, the largest
 * row error of the image its kernel measured (0.3.1); a native catalog's init stays asynchronous. */
typedef struct ebt_catalog {
  const void* data;       /* [n][ld] of dtype (device, caller-owned)                        */
  int32_t dtype, d;
  int64_t n, ld, row_offset; /* row_offset: global id of local row 0 (row-sharded catalogs)  */
  double* gnorm64;        /* [n]                   (state)                                  */
  float* inv32;           /* [round_up(n, 128)]    (state)                                  */
  const void* image;      /* [n][ld_img] f16/bf16  (state, or `data` itself)                */
  const float* cscale;    /* epilogue row scales: inv32 for native images, NULL otherwise   */
  int32_t img_dtype, ld_img, d_pad, native;
  float u_cat;            /* bound on ||image row - row/gnorm||_2 (0: exact native values;
                             measured by ebt_catalog_init; 2^-11 is always a valid value)    */
} ebt_catalog;

size_t ebt_catalog_state_bytes(const void* data, int dtype, int64_t n, int32_t d, int64_t ld);
int ebt_catalog_init(ebt_catalog* cat, const void* data, int dtype, int64_t n, int32_t d,
                     int64_t ld, int64_t row_offset, void* state, size_t state_bytes,
                     void* stream);

/* ---- live updates (0.4.0): replace and append rows in place --------------------------------
 * A catalog that is to grow is initialised with room: `data` holds n_cap >= n rows, `state` is
 * sized by ebt_catalog_state_bytes(data, dtype, n_cap, d, ld) and laid out for n_cap rows, and
 * the first n rows are initialised exactly as ebt_catalog_init would (which is the n_cap == n
 * case); inv32[n .. round_up(n_cap, 128)) = 1.0f. The struct describes the first n rows. */
int ebt_catalog_init_reserved(ebt_catalog* cat, const void* data, int dtype, int64_t n,
                              int64_t n_cap, int32_t d, int64_t ld, int64_t row_offset,
                              void* state, size_t state_bytes, void* stream);

/* Device scratch of ebt_catalog_update_rows for a list of m rows: round_up(8 m, 256) bytes
 * (0 for m <= 0). */
size_t ebt_catalog_update_bytes(int64_t m);

/* Replace m rows: ONE kernel reads each source row once, converts it to the catalog's dtype
 * (round-to-nearest-even; to f16 / bf16 through float, as torch's .to(dtype)), writes it into
 * `data` (the catalog's matrix is written: it must be writable device memory) and recomputes
 * that row's gnorm64, inv32, image row and -- for a non-native catalog -- image error, with the
 * arithmetic and summation order of ebt_catalog_init: afterwards the state is bit-identical to
 * that of a catalog initialised from the edited matrix.
 *   state, state_bytes, n_cap: what ebt_catalog_init(_reserved) was given (n_cap = n for
 *     ebt_catalog_init). The state's layout is derived from n_cap; if cat's pointers do not
 *     match it (a hand-filled struct, another capacity) the call returns EBT_EINVAL. (The
 *     struct does not record the error slot behind the image: an n_cap within the same 32 rows
 *     of the true one moves only that and is not detected. Pass the value given at init.)
 *   rows: HOST pointer, m GLOBAL row ids, strictly ascending, all in [row_offset, row_offset + n).
 *   src: device, m rows of d elements of src_dtype (any of the four), row stride ld_src elements;
 *     it must not overlap `data`.
 *   ws: device scratch of ebt_catalog_update_bytes(m) bytes (the row list).
 * Every argument check (the order and range of `rows` included) runs on the host before any GPU
 * call; a failed check returns EBT_EINVAL and leaves the catalog and *cat unchanged. m == 0 is
 * EBT_OK and does nothing.
 * u_cat: a native catalog's update is fully asynchronous and u_cat stays 0. A non-native one
 * waits for `stream` once to read the error slot back, as ebt_catalog_init does, and sets
 * cat->u_cat to it. The slot holds the RUNNING maximum over every row the catalog ever held: it
 * never decreases, and a replaced row's old error may keep it larger than that of a fresh
 * ebt_catalog_init of the same matrix -- still a valid bound (any value up to 2^-11 is).
 * Ordering: an update is stream-ordered. A batch submitted on the same stream BEFORE the update
 * sees the old catalog, one submitted after it the new one. A batch whose _finish has not
 * returned must be finished before an update is issued: its retries would run after the update
 * and reuse an eps computed from the old u_cat. */
int ebt_catalog_update_rows(ebt_catalog* cat, void* state, size_t state_bytes, int64_t n_cap,
                            const int64_t* rows, int64_t m, const void* src, int src_dtype,
                            int64_t ld_src, void* ws, size_t ws_bytes, void* stream);

/* The same kernel on local rows n .. n + m - 1 (global row_offset + n ..), then cat->n += m.
 * EBT_EINVAL if n + m > n_cap. Workspaces sized by ebt_workspace_bytes for the smaller n may be
 * too small afterwards: size them again (or for n_cap from the start). */
int ebt_catalog_append_rows(ebt_catalog* cat, void* state, size_t state_bytes, int64_t n_cap,
                            int64_t m, const void* src, int src_dtype, int64_t ld_src,
                            void* stream);

/* ---- removal (0.5.0): remove rows in place --------------------------------------------------
 * Removing m distinct rows from a catalog of n rows leaves n' = n - m rows. The holes H are the
 * removed rows below n', ascending; the survivors S are the rows of [n', n) that are not removed,
 * ascending. |H| = |S| = p, row S[i] moves to row H[i], and every other surviving row keeps its
 * number (numpy: c2 = c.copy(); c2[H] = c[S]; c2 = c2[:n']). Sources are all >= n' and
 * destinations all < n', so no move reads what another writes.
 *
 * Device scratch of ebt_catalog_remove_rows for m rows: round_up(16 m, 256) bytes (0 for
 * m <= 0). */
size_t ebt_catalog_remove_bytes(int64_t m);

/* The moves of that rule, on the host (no GPU call). rows: m GLOBAL rows, strictly ascending, all
 * in [row_offset, row_offset + n). from / to: room for m entries each; they receive the p moves
 * as GLOBAL rows (from[i] -> to[i]); both may be NULL. Returns p, or -1 (ebt_last_error) on bad
 * arguments, m >= n included. A caller that keeps row numbers (ratings stored as rows) remaps
 * them with these pairs and drops the removed ones. */
int64_t ebt_catalog_remove_plan(int64_t n, int64_t row_offset, const int64_t* rows, int64_t m,
                                int64_t* from, int64_t* to);

/* Remove m rows by exactly that plan: one copy of the (src, dst) pairs into ws, ONE kernel that
 * copies for each move the d elements of the matrix row (columns d .. ld of `data` are not
 * touched), the image row, gnorm64 and inv32, then inv32[n' .. n) = 1.0f again and cat->n -= m.
 * Nothing is recomputed -- a row's norm and image row depend on its values and on catalog-wide
 * alignment only -- so data, gnorm64, inv32 and the image are bit-identical to those of a catalog
 * initialised from the edited matrix. Only tail rows removed (p == 0): no kernel runs.
 *   cat, state, state_bytes, n_cap: as for ebt_catalog_update_rows.
 *   rows: HOST pointer, m GLOBAL row ids, strictly ascending, all in [row_offset, row_offset + n).
 *   ws: device scratch of ebt_catalog_remove_bytes(m) bytes.
 * Every check (NULL rows, their order and range, m >= n: "cannot remove every row", the
 * workspace size) runs on the host before any GPU call; a failed check returns EBT_EINVAL and
 * leaves *cat and the device state unchanged. m == 0 is EBT_OK and does nothing.
 * u_cat is not touched: the error slot is a running maximum and stays a valid bound, as after
 * ebt_catalog_update_rows; there is no read-back, so for every catalog kind the call is as
 * asynchronous as a native catalog's update (its only host-to-device traffic is the pair list).
 * Ordering: as for the update entries, a removal is stream-ordered, and a batch whose _finish has
 * not returned must be finished before it is issued. Row numbers change: exclusion and liked
 * lists built before the removal must be remapped (ebt_catalog_remove_plan). Workspaces sized by
 * ebt_workspace_bytes for the old n should be sized again. The rows n' .. n of `data` and of the
 * state are free for ebt_catalog_append_rows. */
int ebt_catalog_remove_rows(ebt_catalog* cat, void* state, size_t state_bytes, int64_t n_cap,
                            const int64_t* rows, int64_t m, void* ws, size_t ws_bytes,
                            void* stream);

/* Optional knobs (NULL = defaults; a zero field = its default): kprime = the screen's candidate
 * count k' (default: k + slack for the image's error band), chunk_rows = catalog rows per
 * materialised score chunk of the unfused path (default: 4 GiB of f32 scores),
 * flags = EBT_FLAG_NO_FUSE to disable the fused screen. Results do not depend on them.
 * flags |= EBT_FLAG_LIKED_CHECKED (0.3.2, ebt_cosine_topk / _submit only): the caller has
 * checked its liked CSR on the host -- every user has >= 1 liked row and every row lies in the
 * catalog's [row_offset, row_offset + n) -- so _submit does not read the CSR back (no stream
 * synchronisation: the liked path enqueues asynchronously, as the dense one; the 1/L scales
 * are taken from the offsets on the device, the same float64 values). An unchecked CSR with
 * this flag is undefined behaviour (rows out of range are read). */
#define EBT_FLAG_LIKED_CHECKED 8
typedef struct ebt_options {
  int32_t kprime;
  int32_t flags;
  int64_t chunk_rows;
} ebt_options;

/* Device workspace bytes ebt_cosine_topk needs for a batch of B queries and top-k
 * (0 = invalid arguments). */
size_t ebt_workspace_bytes(const ebt_catalog* cat, int64_t B, int32_t k, const ebt_options* opt);

/* Top-k by cosine for B queries, ordered (score desc, row asc), rows GLOBAL ids.
 * Queries: EITHER dense q [B][ldq] of q_dtype (EBT_F32 / F64 / BF16 / F16; a zero row scores
 * 0 against everything, sklearn's zero-norm guard), OR liked rows (q = NULL): CSR liked_off
 * [B+1] / liked_rows (GLOBAL rows of this catalog) and the query of user b is the mean of its
 * liked rows' normalised vectors (lib.py:51-52). A user with no liked row fails with
 * EBT_EINVAL and sklearn's message ("Found array with 0 sample(s) ..."), as the reference
 * raises ValueError; a liked row outside the catalog fails with EBT_EINVAL.
 * Exclusions (the rated movies, lib.py:48,55): CSR excl_off [B+1] / excl_rows of GLOBAL rows,
 * each segment sorted ascending (checked: EBT_EINVAL otherwise), or both NULL.
 * Output: out_scores float64 [B][k] (within 1e-12 of the float64 reference), out_rows int64
 * [B][k]; slots past the catalog's candidates (k > n minus exclusions) are NaN / -1.
 * ebt_cosine_topk synchronises the stream once (the certificates) and returns when the results
 * are final. The two halves let a caller overlap batches: _submit enqueues the first pass
 * (no synchronisation for dense queries; the liked path reads its CSR offsets on the host) and
 * fills the caller's ebt_pending; _finish waits for THAT batch only (an event), reads its
 * certificates from cert_host (host memory, B + 1 int32) and runs the retries. Pinned
 * cert_host (hipHostMalloc / hipHostRegister, e.g. torch pin_memory) is written by the rescore
 * kernel itself, one store per query across the host link (0.3.3: no copy launch; _submit
 * marks the entries unset first and _finish fails with EBT_EHIP on one that was not
 * delivered); pageable memory gets a copy from the workspace (EBT_HOST_DIRECT=0 forces the
 * copy). Workspace, outputs and cert_host stay in use until _finish returns. timer: NULL or
 * an ebt_timer. */
typedef struct ebt_pending {
  const ebt_catalog* cat;
  ebt_options opt;
  int64_t B, B_pad, chunk;
  int32_t k, k_eff, kprime, flags;
  const int64_t* excl_off;
  const int64_t* excl_rows;
  char* ws;
  size_t ws_bytes;
  double* out_scores;
  int64_t* out_rows;
  int32_t* cert_host;
  void* event;
  void* timer;
  void* stream;
} ebt_pending;
int ebt_cosine_topk(const ebt_catalog* cat, const void* q, int q_dtype, int64_t B, int64_t ldq,
                    const int64_t* liked_off, const int64_t* liked_rows, int32_t k,
                    const int64_t* excl_off, const int64_t* excl_rows, const ebt_options* opt,
                    void* workspace, size_t ws_bytes, double* out_scores, int64_t* out_rows,
                    void* timer, void* stream);
int ebt_cosine_topk_submit(const ebt_catalog* cat, const void* q, int q_dtype, int64_t B,
                           int64_t ldq, const int64_t* liked_off, const int64_t* liked_rows,
                           int32_t k, const int64_t* excl_off, const int64_t* excl_rows,
                           const ebt_options* opt, void* workspace, size_t ws_bytes,
                           double* out_scores,
                           int64_t* out_rows, int32_t* cert_host, ebt_pending* pending,
                           void* timer, void* stream);
int ebt_cosine_topk_finish(ebt_pending* pending);

/* ---- per-query allow masks (0.6.0): top-k within a subset of the catalog rows --------------
 * The reference's candidate set is index.difference(rated) (lib.py:48,55); here it is
 * intersected with a set of allowed rows chosen per query ("within this genre", "only this
 * tenant's items"): the result of a filtered query is the top k of (allowed rows minus excluded
 * rows), same order, same GLOBAL row ids, same float64 scores, NaN / -1 past the candidates.
 *
 * An allow table is uint32 masks[n_masks][words] in device memory, 16-byte aligned, with
 * words = ebt_allow_words(n_rows) = ceil(n_rows / 32) rounded up to a multiple of 4 (every mask
 * row 16-byte aligned); n_rows is the catalog's capacity (n_global for a shard: bits are indexed
 * by GLOBAL row). Row r is allowed in mask m iff masks[m * words + (r >> 5)] >> (r & 31) & 1;
 * rows >= 32 * words are not allowed. mask_id is device int32 [B]: -1 (any negative value) = the
 * query is unfiltered and its scores are not touched; an id >= n_masks masks every row of that
 * query (all slots NaN / -1; nothing is read out of bounds). The result depends on the set of
 * allowed rows only.
 *
 * ebt_allow_from_bool packs uint8 flags[n] (non-zero = allowed; device) into one mask row and
 * zeroes the rest of its `words` words. ebt_allow_set_rows sets (allowed != 0) or clears the
 * bits of the m GLOBAL rows of a device list in one mask row (atomics on the word: duplicates
 * are fine; rows outside [0, 32 * words) are ignored). Both only enqueue on `stream`.
 *
 * ebt_mask_allowed: scores [B][ld_scores] f32 (16-byte aligned, ld_scores % 4 == 0) holds the
 * scores of GLOBAL rows [col_begin, col_end), any col_begin >= 0; every disallowed entry of a
 * filtered query becomes -inf, columns [col_end - col_begin, ld_scores) are left alone. It is
 * the pass the pipeline runs right after ebt_mask_excluded on each score chunk of the unfused
 * path (timed as EBT_STAGE_MASK). Host checks before any GPU call, EBT_EINVAL: NULL pointers,
 * words < 1 or not a multiple of 4, n_masks < 1, 32 * words < col_end.
 *
 * The _allowed entries take their twin's arguments plus `allow`. allow == NULL: exactly the
 * twin, fused screen included. Otherwise the batch runs the unfused path: the entries set
 * EBT_FLAG_NO_FUSE themselves and the caller sizes the workspace with that flag
 * (ebt_workspace_bytes / ebt_cosine_topk_workspace; EBT_ENOMEM when it is too small), and
 * 32 * words must reach row_offset + n. The float64 screen (EBT_FLAG_EXACT) is filtered the same
 * way. _finish takes the same ebt_allow again (ebt_pending, which callers allocate, does not
 * grow): the table and mask_id stay valid and unchanged until it returns. min(k, n) > 4096 (the
 * full-sort path) with a non-NULL allow is EBT_EUNSUPPORTED; ebt_cosine_topk_sharded takes no
 * masks. */
typedef struct ebt_allow {
  const uint32_t* masks;    /* device [n_masks][words] */
  int64_t words;            /* ebt_allow_words(capacity) */
  int32_t n_masks;
  const int32_t* mask_id;   /* device [B]: mask of query b, -1 = unfiltered */
} ebt_allow;
int64_t ebt_allow_words(int64_t n_rows);
int ebt_allow_from_bool(const uint8_t* flags, int64_t n, uint32_t* mask_row, int64_t words,
                        void* stream);
int ebt_allow_set_rows(uint32_t* mask_row, int64_t words, const int64_t* rows, int64_t m,
                       int allowed, void* stream);
int ebt_mask_allowed(float* scores, int64_t ld_scores, int64_t B, int64_t col_begin,
                     int64_t col_end, const ebt_allow* allow, void* stream);
int ebt_cosine_topk_prepared_allowed(
    const double* q64, const void* qimg, const float* qscale, const float* eps, int64_t B,
    int64_t B_pad, const void* cat, int dtype, int64_t ld, const double* gnorm64,
    const void* cimg, const float* cscale, int img_dtype, int32_t ld_img, int64_t n_rows,
    int32_t d, int32_t d_pad, int64_t row_offset, const int64_t* excl_off,
    const int64_t* excl_rows, int32_t k, int32_t kprime, int64_t chunk_rows, int flags,
    void* workspace, size_t ws_bytes, double* out_scores, int64_t* out_rows, int32_t* certified,
    void* timer, void* stream, const ebt_allow* allow);
int ebt_cosine_topk_allowed(const ebt_catalog* cat, const void* q, int q_dtype, int64_t B,
                            int64_t ldq, const int64_t* liked_off, const int64_t* liked_rows,
                            int32_t k, const int64_t* excl_off, const int64_t* excl_rows,
                            const ebt_options* opt, void* workspace, size_t ws_bytes,
                            double* out_scores, int64_t* out_rows, void* timer, void* stream,
                            const ebt_allow* allow);
int ebt_cosine_topk_allowed_submit(const ebt_catalog* cat, const void* q, int q_dtype, int64_t B,
                                   int64_t ldq, const int64_t* liked_off,
                                   const int64_t* liked_rows, int32_t k, const int64_t* excl_off,
                                   const int64_t* excl_rows, const ebt_options* opt,
                                   void* workspace, size_t ws_bytes, double* out_scores,
                                   int64_t* out_rows, int32_t* cert_host, ebt_pending* pending,
                                   void* timer, void* stream, const ebt_allow* allow);
int ebt_cosine_topk_allowed_finish(ebt_pending* pending, const ebt_allow* allow);

/* ---- materialised sub-catalogs (0.7.0): a sparse mask scored over its own rows --------------
 * The _allowed entries above score every catalog row and then mask: their cost does not fall
 * with the mask's density. A row's state does not depend on where the row is -- its norm, inverse
 * norm and image row are functions of its values (the fact ebt_catalog_remove_rows relies on) --
 * so the m allowed rows of one mask can be copied ONCE into a dense catalog of their own, the
 * SUB-CATALOG, whose row i is the i-th allowed row in ascending order. Every scoring entry runs
 * over it unchanged (ebt_cosine_topk and its fused screen included, allow == NULL), on m rows
 * instead of n. The map sub row -> GLOBAL row is strictly increasing, so the order (score desc,
 * row asc) is kept, and the float64 scores are those of the same rows in the parent, bit for bit
 * (the rescore reads the same values and norms; give the copy the parent's row alignment, see
 * ld_out). A caller keeps: the row list [m], the rank prefix [words], the sub-catalog's buffers.
 * The copy is a snapshot: after the mask or the parent changes (ebt_allow_set_rows,
 * ebt_allow_from_bool, ebt_catalog_update_rows / _append_rows / _remove_rows) build it again.
 * Recipe for one filtered batch: dense queries go to ebt_cosine_topk(sub, ...) as they are;
 * liked queries are prepared against the PARENT (liked rows need not be allowed:
 * ebt_query_liked_sum, ebt_scale_rows_f64, ebt_query_image with the parent's u_cat) and run
 * through ebt_cosine_topk_prepared over the sub-catalog; exclusions go through
 * ebt_sub_exclusions; result rows come back through ebt_sub_rows_to_global.
 *
 * In all of these a mask row is uint32 [words] as in struct ebt_allow: words a positive multiple
 * of 4, at most 2^26; 16-byte alignment is not required here. Only rows [0, n_rows) count: bits
 * at or above n_rows are ignored (ebt_allow_from_bool can leave them set past the catalog's n).
 * Host checks run before any GPU call and return EBT_EINVAL: NULL pointers, words not a positive
 * multiple of 4, n_rows < 0 or > 32 * words, a workspace that is too small. Everything is
 * enqueued on `stream`; nothing waits for it.
 *
 * ebt_allow_count: *count_out (device int64) = the allowed rows of the mask row below n_rows.
 *
 * ebt_allow_rows: the stream compaction of one mask row. rows_out (device int64 [cap]) receives
 * the allowed rows < n_rows, ascending; *count_out (device int64) how many there are -- entries
 * past cap are counted, not written (cap = 0: count and rank only, rows_out may be NULL);
 * rank_out (device uint32 [words]) receives for each word the number of allowed rows < n_rows in
 * all earlier words (the exclusive prefix of the words' popcounts). Two launches: per-workgroup
 * popcount totals into ws (ebt_allow_rows_bytes(words) bytes; 0 = invalid words), then each
 * workgroup sums the totals before it and scans its own words. Output positions are computed,
 * not claimed: the result is deterministic and no atomic is used. */
int ebt_allow_count(const uint32_t* mask_row, int64_t words, int64_t n_rows, int64_t* count_out,
                    void* stream);
size_t ebt_allow_rows_bytes(int64_t words);
int ebt_allow_rows(const uint32_t* mask_row, int64_t words, int64_t n_rows, int64_t* rows_out,
                   int64_t cap, uint32_t* rank_out, int64_t* count_out, void* ws, size_t ws_bytes,
                   void* stream);

/* The gather: ONE kernel, a wave per output row. Output row i is the parent's row rows[i] (device
 * list of m GLOBAL rows, any order, duplicates allowed): its d matrix elements into
 * data_out[i][0 .. d) (row stride ld_out elements; columns d .. ld_out are not written), its
 * image row into image_out[i][0 .. ld_img) (ld_img = the parent's), gnorm64 and inv32; and
 * inv32_out[m .. round_up(m, 128)) = 1.0f. Nothing is recomputed: the copies are bit-identical
 * to what ebt_catalog_init computes for a matrix made of those rows with the parent's alignment.
 * A rows[i] outside [row_offset, row_offset + n) is never followed: that output row is zero-filled
 * with gnorm 1 and inv32 1, and nothing is read out of bounds.
 *   data_out [m][ld_out] of the parent's dtype, gnorm_out [m], inv32_out [round_up(m, 128)],
 *   image_out [m][ld_img] 16-bit, 16-byte aligned: device buffers of the caller, which must
 *   outlive *sub. When the parent's matrix is its own image (parent->image == parent->data)
 *   image_out is ignored (NULL), the sub-catalog's image is data_out, and ld_out must be a
 *   multiple of 64 with data_out 16-byte aligned.
 *   ld_out: the rescore picks its 16-byte form when the matrix is 16-byte aligned with
 *   ld * elem % 16 == 0 and d * elem % 16 == 0; give the copy the same property as the parent
 *   (ld_out = d, or the parent's ld, does when the parent is so aligned) and scores stay bitwise
 *   equal; any ld_out >= d is correct.
 * *sub (host) is filled before the call returns: n = m, row_offset = 0, data / ld / gnorm64 /
 * inv32 / image the buffers above, dtype, d, img_dtype, d_pad and native the parent's, ld_img the
 * parent's (ld_out when the matrix is its own image), cscale = inv32_out for a native parent and
 * NULL otherwise, u_cat the parent's (a bound over all its rows, so over the copied ones).
 * EBT_EINVAL before any GPU call: NULL pointers, m < 1, ld_out < d, a parent whose matrix is its
 * own image with ld_out % 64 != 0, image_out NULL for a parent with an image of its own. */
int ebt_catalog_gather_rows(const ebt_catalog* parent, const int64_t* rows, int64_t m,
                            void* data_out, int64_t ld_out, double* gnorm_out, float* inv32_out,
                            void* image_out, ebt_catalog* sub, void* stream);

/* An exclusion CSR of GLOBAL rows (off [B + 1] positions into rows [nnz], each segment ascending,
 * off[0] may be > 0) in the sub-catalog's row numbers: an allowed row r < n_rows becomes
 * rank[r >> 5] + popcount(word[r >> 5] & ((1u << (r & 31)) - 1)), every other row is dropped.
 * The output is a compact CSR, off_out [B + 1] with off_out[0] = 0 and rows_out (room for nnz
 * entries), each segment still ascending (the map is increasing). Three launches: count per
 * query, scan, write; ws of ebt_sub_exclusions_bytes(B, nnz) bytes (0 for B < 1, nnz < 0 or
 * either above 2^31). Offsets pointing outside [0, nnz) are clipped, never followed. */
size_t ebt_sub_exclusions_bytes(int64_t B, int64_t nnz);
int ebt_sub_exclusions(const uint32_t* mask_row, int64_t words, const uint32_t* rank,
                       int64_t n_rows, const int64_t* off, const int64_t* rows, int64_t B,
                       int64_t nnz, int64_t* off_out, int64_t* rows_out, void* ws,
                       size_t ws_bytes, void* stream);

/* Result rows of a sub-catalog back to GLOBAL rows, in place (device int64 [count]): r < 0 stays
 * -1, 0 <= r < m becomes list[r] (ebt_allow_rows' rows_out), anything else becomes -1. */
int ebt_sub_rows_to_global(int64_t* rows_inout, int64_t count, const int64_t* list, int64_t m,
                           void* stream);

/* ---- row-sharded catalog, self-contained: one call per batch on every rank ---------------
 * The per-shard protocol of robot_ebert_amd/distributed.py (score_topk_sharded_local_stages)
 * inside the library, for a host without Python: every rank holds one shard (an ebt_catalog
 * whose row_offset is the shard's first GLOBAL row) and calls ebt_cosine_topk_sharded with the
 * same queries, k and exclusions; every rank returns the same GLOBAL top-k, equal to
 * ebt_cosine_topk over the whole catalog (rows bit-exact, float64 scores). For liked queries
 * the query is the same up to float64 round-off of its sum: each shard sums its own liked rows
 * and the partial sums are added in rank order, so the additions are grouped by shard (equal to
 * the single-GPU sum when no shard after the first holds two of a user's liked rows); rows
 * within round-off of a tie may then swap -- as they may against the reference itself, which
 * averages the per-row cosine scores instead of the rows (lib.py:51-52). Per batch:
 *   query prep (liked rows: each shard sums its own, one all-gather of the [B][d] float64
 *   partial sums completes the means); when the shards are small (<= 200K rows, >= 2 ranks, the
 *   fused screen) a catalog-wide screening threshold from every shard's sample maxima (one
 *   all-gather); the shard's screen; the catalog-wide floor of the k-th exact score (one
 *   all-gather of [B][k+1] float32) so each shard rescores only rows that can enter the global
 *   top k (each shard sends its ebt_shard_list_width best approx, [B][w+1] float32); the
 *   float64 rescore + certificate; the local retries (no collective: every rank issues the same
 *   all-gathers in the same order whatever its retries); one all-gather of the shards' entries
 *   above that floor (ebt_shard_pack: int32 rows behind per-query starts) and the merge
 *   (ebt_merge_packed) -- or, when the compact form does not apply or a rank's entries exceed
 *   its capacity, two all-gathers of the full [B][k] lists and ebt_merge_topk.
 * The caller supplies the collective, an all-gather over its communicator:
 *   all_gather(ctx, send, recv, bytes, stream): recv (device, world * bytes) receives every
 *   rank's `bytes` from send (device) in rank order. It is called after the work producing
 *   `send` has been enqueued on `stream`, and the library enqueues work reading `recv` on
 *   `stream` right after it returns: a stream-ordered collective (RCCL: ncclAllGather(send,
 *   recv, bytes, ncclInt8, comm, stream)) or a blocking one both work.
 *   It returns 0 on success; anything else fails the call with EBT_EHIP (the other ranks are
 *   then left in their next all_gather: the caller's collective timeout must end them).
 * Limits: k <= 4096 (the merge); B, k, the queries and the exclusions equal on every rank
 * (argument errors are then detected alike everywhere before the first collective). The call
 * returns when the results are final. Workspace: ebt_sharded_workspace_bytes (device). */
typedef int (*ebt_allgather_fn)(void* ctx, const void* send, void* recv, size_t bytes,
                                void* stream);
/* Optional: buf[0 .. count) (device float64) <- the sum over ranks of every rank's buf, in place
 * (RCCL: ncclAllReduce(buf, buf, count, ncclFloat64, ncclSum, comm, stream)). The liked path's
 * partial sums use it when it is set -- about 2 / R of the all-gather's volume; the sum's order
 * of additions is then the collective's, a float64 round-off-level difference -- else an
 * all-gather of every rank's partial sums added in rank order. NULL = not provided. */
typedef int (*ebt_allreduce_f64_fn)(void* ctx, double* buf, size_t count, void* stream);
/* Zero-initialise (`ebt_comm c = {0};`, or memset) before filling it in: a field a caller built
 * against an older layout does not set must read NULL (see ebt_version). */
typedef struct ebt_comm {
  int32_t rank, world;
  int64_t n_global;           /* rows of the whole catalog: every shard's row_offset + n <= it */
  ebt_allgather_fn all_gather;
  void* ctx;
  ebt_allreduce_f64_fn all_reduce_f64;  /* optional (NULL), same ctx */
} ebt_comm;
/* An RCCL communicator for an ebt_comm: the library opens librccl.so.1 at first use (it does not
 * link it). Rank 0 calls ebt_rccl_unique_id (128 bytes) and hands the id to every rank out of
 * band (e.g. a torch.distributed broadcast); each rank calls ebt_rccl_comm_init with its HIP
 * device current; then comm.all_gather = ebt_rccl_all_gather, comm.all_reduce_f64 =
 * ebt_rccl_all_reduce_f64, comm.ctx = the handle (ncclAllGather of `bytes` int8, ncclAllReduce
 * of float64 sums, on `stream`). EBT_EUNSUPPORTED when RCCL cannot be loaded. */
int ebt_rccl_unique_id(void* id_out, size_t bytes);
int ebt_rccl_comm_init(const void* id, int32_t rank, int32_t world, void** comm_out);
int ebt_rccl_comm_destroy(void* comm);
int ebt_rccl_all_gather(void* comm, const void* send, void* recv, size_t bytes, void* stream);
int ebt_rccl_all_reduce_f64(void* comm, double* buf, size_t count, void* stream);
size_t ebt_sharded_workspace_bytes(const ebt_catalog* cat, const ebt_comm* comm, int64_t B,
                                   int32_t k, const ebt_options* opt);
/* The same in three calls, so that a caller can keep batches in flight (the collectives and
 * the host's waits of one batch behind the GPU work of the next):
 *   _submit enqueues query prep, the threshold and floor all-gathers, the screen, the rescore
 *     and the certificates into host[0 .. B] (caller's host memory, B + 2 int32; pinned: the
 *     rescore's own stores, else a copy -- as ebt_cosine_topk_submit) and fills *pending;
 *   _finish waits for THAT batch's certificates, runs the shard's local retries, packs the
 *     shard's entries above the catalog-wide floor (ebt_shard_pack), all-gathers them, merges
 *     (ebt_merge_packed) into out_scores / out_rows on the stream and brings the merge's
 *     "incomplete" flag to host[B + 1] (pinned: written by the merge itself);
 *   _wait waits for that flag (an event) and, when a rank's entries did not fit its packed
 *     capacity, re-merges from the full lists (two more all-gathers: every rank sees the same
 *     flag). The results are final when _wait returns.
 * Every rank must make the same sequence of calls (each issues collectives). Workspace, host
 * buffer and outputs belong to the batch until its _wait returns, so a pipelined caller cycles
 * through (at least) three workspaces, e.g. per step: submit(i), finish(i-1), wait(i-2).
 * ebt_cosine_topk_sharded = submit + finish + wait. */
typedef struct ebt_sharded_pending {
  ebt_pending local;  /* the shard's own first pass and retries */
  ebt_comm comm;
  double* out_scores;
  int64_t* out_rows;
  int32_t* host;
  void* event;
  int32_t stage;      /* 1 submitted, 2 finished, 0 done */
} ebt_sharded_pending;
int ebt_cosine_topk_sharded_submit(const ebt_catalog* cat, const ebt_comm* comm, const void* q,
                                   int q_dtype, int64_t B, int64_t ldq,
                                   const int64_t* liked_off, const int64_t* liked_rows,
                                   int32_t k, const int64_t* excl_off, const int64_t* excl_rows,
                                   const ebt_options* opt, void* workspace, size_t ws_bytes,
                                   double* out_scores, int64_t* out_rows, int32_t* host,
                                   ebt_sharded_pending* pending, void* timer, void* stream);
int ebt_cosine_topk_sharded_finish(ebt_sharded_pending* pending);
int ebt_cosine_topk_sharded_wait(ebt_sharded_pending* pending);
int ebt_cosine_topk_sharded(const ebt_catalog* cat, const ebt_comm* comm, const void* q,
                            int q_dtype, int64_t B, int64_t ldq, const int64_t* liked_off,
                            const int64_t* liked_rows, int32_t k, const int64_t* excl_off,
                            const int64_t* excl_rows, const ebt_options* opt, void* workspace,
                            size_t ws_bytes, double* out_scores, int64_t* out_rows, void* timer,
                            void* stream);

/* ---- weighted and negative feedback (0.8.0): per-row weights on liked-row queries -----------
 * The reference turns a rating into a 0/1 vote (lib.py:47-52: rating >= LIKED_MOVIE_SCORE is a
 * liked row, the query is the plain mean of the liked rows) and uses everything below the
 * threshold only as an exclusion. These entries generalise that mean: with weights w_l (device
 * float64, one per entry of liked_rows, in the same order) on the liked rows r_l of query b,
 * l in [liked_off[b], liked_off[b+1]),
 *   score_b(j) = ( sum_l w_l cos(x_{r_l}, x_j) ) / W_b,       W_b = sum_l |w_l|
 *   q64[b]     = ( sum_l w_l (x_{r_l} / gnorm64[r_l]) ) * (1 / W_b).
 * A weight may be negative ("unlike this": the row pushes away), and liked_rows may repeat a
 * row (each entry is its own term). |q64[b]| <= 1 as for the mean (the triangle inequality over
 * unit vectors, divided by W_b), so the screen, its eps, the certificate, the rescore and every
 * retry run unchanged on q64: only the query prep sees the weights.
 * The arithmetic is fixed, so that results can be compared bitwise: the per-element term is the
 * rounded product w * (x / g) (no fused multiply-add), added in CSR order -- the element and
 * the 16-byte-chunk kernels give the same bits, and weights of 1.0 give ebt_query_liked_sum's;
 * W_b is the sequential float64 sum of |w_l| in CSR order; the scale is 1.0 / W_b, applied as
 * ebt_scale_rows_f64 applies 1 / L. The host check and the device (EBT_FLAG_LIKED_CHECKED)
 * compute the identical W_b. Hence: all weights 1.0 = the unweighted call; weights times a power
 * of two = the same result; a 0.0 weight = that entry removed.
 *
 * ebt_query_liked_wsum: ebt_query_liked_sum with the weights (still a SUM: the caller scales).
 * ebt_cosine_topk_weighted / _weighted_submit: the arguments of ebt_cosine_topk_allowed /
 * _allowed_submit (allow may be NULL) plus liked_w. liked_w == NULL is exactly that entry: the
 * same kernels, the same bits. liked_w with dense q is EBT_EINVAL. A batch is finished with
 * ebt_cosine_topk_allowed_finish (ebt_pending holds nothing of the liked CSR). Found before any
 * scoring work, EBT_EINVAL with a message naming the query: a NaN or infinite weight, W_b == 0
 * (a query with no liked row gives sklearn's message first, as always). With
 * EBT_FLAG_LIKED_CHECKED the caller vouches for the weights as well (all finite, W_b > 0):
 * nothing is read back, the submit stays asynchronous, 1 / W_b is computed on the device.
 * The weights are the caller's device memory, valid for as long as liked_rows must be; the
 * per-query scale uses the liked path's existing scratch, so workspace sizes do not change
 * (ebt_workspace_bytes / ebt_sharded_workspace_bytes).
 * ebt_cosine_topk_sharded_weighted / _sharded_weighted_submit: every rank passes the same
 * GLOBAL CSR and the same weights; each shard sums its own rows weighted, the partial sums are
 * exchanged exactly as the unweighted ones (the caller's all-reduce, or the gather added in rank
 * order), then scaled by 1 / W_b, which every rank computes from the full list. _finish and
 * _wait are the unweighted entries'. */
int ebt_query_liked_wsum(const void* cat, int dtype, int32_t d, int64_t ld,
                         const double* gnorm64_cat, int64_t B, const int64_t* liked_off,
                         const int64_t* liked_rows, const double* liked_w, double* q64,
                         void* stream);
int ebt_cosine_topk_weighted(const ebt_catalog* cat, const void* q, int q_dtype, int64_t B,
                             int64_t ldq, const int64_t* liked_off, const int64_t* liked_rows,
                             int32_t k, const int64_t* excl_off, const int64_t* excl_rows,
                             const ebt_options* opt, void* workspace, size_t ws_bytes,
                             double* out_scores, int64_t* out_rows, void* timer, void* stream,
                             const ebt_allow* allow, const double* liked_w);
int ebt_cosine_topk_weighted_submit(const ebt_catalog* cat, const void* q, int q_dtype, int64_t B,
                                    int64_t ldq, const int64_t* liked_off,
                                    const int64_t* liked_rows, int32_t k, const int64_t* excl_off,
                                    const int64_t* excl_rows, const ebt_options* opt,
                                    void* workspace, size_t ws_bytes, double* out_scores,
                                    int64_t* out_rows, int32_t* cert_host, ebt_pending* pending,
                                    void* timer, void* stream, const ebt_allow* allow,
                                    const double* liked_w);
int ebt_cosine_topk_sharded_weighted(const ebt_catalog* cat, const ebt_comm* comm, const void* q,
                                     int q_dtype, int64_t B, int64_t ldq,
                                     const int64_t* liked_off, const int64_t* liked_rows,
                                     int32_t k, const int64_t* excl_off,
                                     const int64_t* excl_rows, const ebt_options* opt,
                                     void* workspace, size_t ws_bytes, double* out_scores,
                                     int64_t* out_rows, void* timer, void* stream,
                                     const double* liked_w);
int ebt_cosine_topk_sharded_weighted_submit(
    const ebt_catalog* cat, const ebt_comm* comm, const void* q, int q_dtype, int64_t B,
    int64_t ldq, const int64_t* liked_off, const int64_t* liked_rows, int32_t k,
    const int64_t* excl_off, const int64_t* excl_rows, const ebt_options* opt, void* workspace,
    size_t ws_bytes, double* out_scores, int64_t* out_rows, int32_t* host,
    ebt_sharded_pending* pending, void* timer, void* stream, const double* liked_w);

/* ---- explanations (0.9.0): the per-liked-row contributions to each returned score -----------
 * The reference scores a user by cosine_similarity(catalog.loc[liked], catalog).mean(axis=0)
 * (lib.py:51-52): a returned score is a sum of one term per liked row,
 *   score_b(j) = sum_l contrib(b, j, l),
 *   contrib(b, j, l) = ( w_l * ( (x_{r_l} . x_j) / (g_{r_l} * g_j) ) ) * (1 / W_b),
 * with w_l = 1 and W_b = L_b unweighted, W_b = sum_l |w_l| with weights (0.8.0). The search
 * entries fold the liked rows into one query vector before their GEMM and never hold the terms;
 * these entries compute them afterwards for the rows a search returned -- the reference's matrix
 * pairwise_similarities restricted to the returned columns, before .mean, times w_l / W_b -- and
 * pick the m largest (or smallest) per returned row: "because you liked X and Y", "despite Z".
 *
 * Inputs: the liked CSR of the search (liked_off [B + 1], liked_rows, liked_w or NULL; GLOBAL
 * rows, any order, a row may repeat: every entry is its own term) and rows [B][k], the GLOBAL
 * result rows (-1 = an empty slot), all of ONE unsharded catalog: rows [row_offset,
 * row_offset + n). Results of masked and sub-catalog searches qualify (they are parent rows).
 *
 * ebt_liked_contrib: out[k * liked_off[b] + j * L_b + l] = contrib(b, j, l), l the position in
 * query b's list (a CSR-shaped matrix: k * nnz float64 in all). All arithmetic is float64; g is
 * the catalog's guarded gnorm64, so a zero-norm row contributes exactly 0 (sklearn); W_b is the
 * sequential sum of |w_l| in CSR order, as in 0.8.0, and the four operations of the formula are
 * rounded one at a time in the order written. The dot products run on the float64 MFMA in a
 * fixed order that depends on d and the dtype only (csrc/explain.hip), so query b's values are
 * bitwise the same alone or in any batch, with weights 1.0 or liked_w == NULL, and under any
 * power-of-two scaling of the weights. Empty result slots give NaN. A liked or result row outside
 * the catalog is never read: status[b] = -2 and every output of that query is NaN; otherwise
 * status[b] = 1 (device int32 [B]; nothing is read back, the call only enqueues).
 *
 * ebt_explain_select: from each (b, j) segment of L_b values, the m best in the order (value
 * desc, position asc), or (value asc, position asc) with largest == 0; -0 equals +0; a NaN is
 * never selected. out_val [B][k][m] float64 (NaN padded), out_pos [B][k][m] int32 position in
 * query b's list (-1 padded; the unambiguous handle when a list repeats a row), out_row
 * [B][k][m] int64 = liked_rows at that position (-1 padded), out_total [B][k] = the sequential
 * float64 sum of the segment in list order (NULL: not computed). 1 <= m <= EBT_EXPLAIN_M_MAX.
 *
 * ebt_explain_topk: the two above over a caller's workspace of ebt_explain_workspace_bytes(nnz, k)
 * bytes (the matrix: 8 * k * nnz rounded up to 256, at least 256; 0 for nnz < 0 or k < 1), nnz =
 * liked_off[B] as the caller knows it on the host.
 *
 * Found on the host before any GPU call, EBT_EINVAL with a message: a null pointer, k < 1, m out
 * of range, a workspace that is too small. No timer stage is recorded. */
#define EBT_EXPLAIN_M_MAX 64
size_t ebt_explain_workspace_bytes(int64_t nnz, int32_t k);
int ebt_liked_contrib(const ebt_catalog* cat, int64_t B, const int64_t* liked_off,
                      const int64_t* liked_rows, const double* liked_w, const int64_t* rows,
                      int32_t k, double* out, int32_t* status, void* stream);
int ebt_explain_select(const double* contrib, int64_t B, const int64_t* liked_off,
                       const int64_t* liked_rows, int32_t k, int32_t m, int largest,
                       double* out_val, int32_t* out_pos, int64_t* out_row, double* out_total,
                       void* stream);
int ebt_explain_topk(const ebt_catalog* cat, int64_t B, const int64_t* liked_off,
                     const int64_t* liked_rows, const double* liked_w, int64_t nnz,
                     const int64_t* rows, int32_t k, int32_t m, int largest, void* workspace,
                     size_t ws_bytes, double* out_val, int32_t* out_pos, int64_t* out_row,
                     double* out_total, int32_t* status, void* stream);

/* ---- diversified top-k (0.10.0): greedy maximal marginal relevance over a candidate pool -----
 * The reference sorts by score and cuts at k (lib.py:51-55), so the k best rows may be near
 * copies of one another. These entries re-rank a POOL of p > k rows per query: k picks, each
 * maximising lam * relevance - (1 - lam) * (largest cosine to a row already picked). The cosine
 * between two catalog rows is lib.py:51's quantity, used among the results. Everything is
 * float64 and every operation is rounded one at a time.
 *
 * Inputs per query b: rows [B][p], GLOBAL rows of ONE unsharded catalog (rows [row_offset,
 * row_offset + n)), -1 = an empty slot, and rel [B][p], their relevances -- what a search with
 * k = p returned is the intended input (results of masked and sub-catalog searches are parent
 * rows and qualify); any list is legal. A slot is a CANDIDATE iff its row is >= 0 and its rel is
 * not NaN.
 *
 * ebt_pool_gram: gram[(b * p + i) * p + j] = S(b, i, j) = (x_i . x_j) / (g_i * g_j), g the
 * catalog's guarded gnorm64, so a zero-norm row has S = 0 against everything, itself included
 * (sklearn); NaN where slot i or j is empty. The dot products run on the float64 MFMA in a fixed
 * order that depends on d and the dtype only (csrc/diversify.hip, the rule of csrc/explain.hip):
 * query b's matrix has the same bits alone or in any batch, S(b, i, j) and S(b, j, i) have the
 * same bits, and permuting the pool permutes the matrix bitwise. A pool row outside the catalog
 * is never read: status[b] = -2 and every value of that query is NaN; otherwise status[b] = 1
 * (device int32 [B]; nothing is read back, the call only enqueues).
 *
 * ebt_mmr_select, with oml = 1.0 - lam computed once:
 *   pen_i = +0.0 for every i
 *   for t = 0 .. k-1:
 *     v_i = (lam * rel_i) - (oml * pen_i)         over the candidates not yet picked
 *     s   = arg max by (v desc, position asc)     (-0 equals +0; a NaN v is never picked)
 *     out_pos[b][t] = s; out_rows[b][t] = rows[b][s]; out_rel[b][t] = rel_s (the input's bits);
 *     out_mmr[b][t] = v_s
 *     pen_i = S(b, s, i) if t == 0, else S(b, s, i) > pen_i ? S(b, s, i) : pen_i
 * Slots past the candidates read -1 / -1 / NaN / NaN. With lam == 1 the result is the candidates
 * ordered by (rel desc, position asc): for a search result its own first k, bit for bit.
 * 1 <= k <= p <= EBT_MMR_POOL_MAX; lam is a host double in [0, 1]. status may be NULL; a query
 * with status[b] < 0 gets all-empty outputs.
 *
 * ebt_mmr_topk: the two above over a caller's workspace of ebt_mmr_workspace_bytes(B, p) bytes
 * (the matrices: 8 * B * p * p rounded up to 256, at least 256; 0 for B < 1, p < 1,
 * p > EBT_MMR_POOL_MAX or a product that overflows).
 *
 * Found on the host before any GPU call, EBT_EINVAL with a message that starts with the entry's
 * name: a null pointer, p or k out of range, lam outside [0, 1] or NaN, a catalog whose ld < d,
 * a workspace that is too small. No timer stage is recorded. */
#define EBT_MMR_POOL_MAX 512
size_t ebt_mmr_workspace_bytes(int64_t B, int32_t p);
int ebt_pool_gram(const ebt_catalog* cat, int64_t B, const int64_t* rows, int32_t p,
                  double* gram, int32_t* status, void* stream);
int ebt_mmr_select(const double* gram, const double* rel, const int64_t* rows, int64_t B,
                   int32_t p, int32_t k, double lam, const int32_t* status,
                   int32_t* out_pos, int64_t* out_rows, double* out_rel, double* out_mmr,
                   void* stream);
int ebt_mmr_topk(const ebt_catalog* cat, int64_t B, const double* rel, const int64_t* rows,
                 int32_t p, int32_t k, double lam, void* workspace, size_t ws_bytes,
                 int32_t* out_pos, int64_t* out_rows, double* out_rel, double* out_mmr,
                 int32_t* status, void* stream);

/* ---- multi-interest top-k (0.11.0): cluster the liked rows, interleave the answers ------------
 * The reference scores a user as the mean cosine to everything they liked (lib.py:51-52), so a
 * user with several distinct tastes is searched at the centroid of those tastes. These entries
 * group the liked rows of a query into up to c clusters and merge the top-k lists searched once
 * per cluster, each cluster taking output slots in proportion to its size.
 *
 * rows [B][p]: GLOBAL rows of ONE unsharded catalog, -1 = an empty slot anywhere in the list,
 * 1 <= p <= EBT_MMR_POOL_MAX. The "position" of a row is its slot in that list.
 *
 * ebt_interest_cluster, per query, with S = that query's gram [p][p] (what ebt_pool_gram wrote:
 * bitwise symmetric). Everything is float64 and every operation is rounded on its own; -0 equals
 * +0 in comparisons:
 *
 *   valid_i = rows[i] >= 0;  L = #valid;  c_eff = min(c, L)
 *   L == 0: label = -1, size = 0, medoid = -1, iters = 0
 *   tot_i = +0.0; for j ascending over valid j: tot_i = tot_i + S(i, j)            (valid i)
 *   seed_0 = arg max by (tot desc, position asc);  near_i = S(seed_0, i)
 *   for m = 1 .. c_eff-1:
 *       seed_m = arg min over valid non-seed i by (near asc, position asc)
 *       near_i = S(seed_m, i) > near_i ? S(seed_m, i) : near_i
 *   label_i = arg max over m < c_eff by (S(seed_m, i) desc, m asc);  label_{seed_m} = m
 *   PASS(label): n_m = #{i: label_i = m}
 *                acc_{i,m} = +0.0; for j ascending over valid j: acc_{i,label_j} = acc_{i,label_j} + S(i, j)
 *                mean_{i,m} = acc_{i,m} / (double) n_m           (only for n_m > 0)
 *   for it = 1 .. EBT_INTEREST_ITERS:
 *       PASS(label); new_i = arg max over m with n_m > 0 by (mean_{i,m} desc, m asc)
 *       iters = it;  if new == label everywhere: break;  label = new
 *   PASS(label) once more if the loop ended at the cap (otherwise the last pass's values are the
 *   final ones)
 *   medoid_m = arg max over the members i of m by (mean_{i,m} desc, position asc); -1 if n_m == 0
 *   renumber the clusters by (n desc, lowest member position asc), empty ones last; outputs use
 *   the new numbers; out_size[m] = n_m (0 for m >= the number of non-empty clusters);
 *   out_label = -1 on empty slots
 *
 * mean_{i,m} is the reference's own score of row i against the list "cluster m" (lib.py:51-52):
 * a liked row joins the cluster that would recommend it most strongly. out_medoid holds
 * positions. The result does not depend on where the -1 slots are, on how far the list is padded
 * or on the other queries of the batch. (A NaN in S between valid slots is outside the contract:
 * it ranks last in every arg max / arg min and the outputs stay within range.) status may be
 * NULL; a query with status[b] < 0 gets all-empty outputs.
 *
 * ebt_liked_interests: ebt_pool_gram into a caller's workspace of
 * ebt_interest_workspace_bytes(B, p) = ebt_mmr_workspace_bytes(B, p) bytes, then
 * ebt_interest_cluster (ebt_mmr_topk's composition). A row outside the catalog is never read:
 * status[b] = -2 and that query's outputs are all empty.
 *
 * ebt_interest_interleave, per query: cluster m gets output slots in proportion to size[m] by
 * the highest-averages (D'Hondt) rule in integer arithmetic; list_rows / list_scores [B][c][k]
 * are the per-cluster results (-1 / anything = an empty slot):
 *
 *   taken_m = 0; next_m = 0
 *   for t = 0 .. k-1:
 *       every m: while next_m < k and (list_rows[m][next_m] < 0 or that row was already
 *                emitted): next_m++
 *       live = {m: size_m > 0 and next_m < k};  none: stop
 *       m* = the live m with the largest size_m / (taken_m + 1), compared exactly: a beats b iff
 *            size_a * (taken_b + 1) > size_b * (taken_a + 1), or these are equal and a < b (int64)
 *       out_rows[t] = list_rows[m*][next_m*]; out_scores[t] = its score, the input's bits;
 *       out_cluster[t] = m*; out_pos[t] = next_m*;  taken_m*++; next_m*++
 *   slots past the stop: -1 / NaN / -1 / -1
 *
 * Found on the host before any GPU call, EBT_EINVAL with a message that starts with the entry's
 * name: a null pointer, p outside [1, EBT_MMR_POOL_MAX], c outside [1, EBT_INTEREST_MAX], k
 * outside [1, EBT_INTEREST_K_MAX], B < 0 (for the clustering also B > 4 * (2^31 - 1): one wave
 * per query, four per workgroup), a catalog whose ld < d, a workspace that is too small.
 * B == 0 returns EBT_OK without a launch. No timer stage is recorded. */
#define EBT_INTEREST_MAX 8      /* clusters per query */
#define EBT_INTEREST_ITERS 16   /* reassignment passes */
#define EBT_INTEREST_K_MAX 512
size_t ebt_interest_workspace_bytes(int64_t B, int32_t p);
int ebt_interest_cluster(const double* gram, const int64_t* rows, int64_t B, int32_t p, int32_t c,
                         const int32_t* status, int32_t* out_label, int32_t* out_size,
                         int32_t* out_medoid, int32_t* out_iters, void* stream);
int ebt_liked_interests(const ebt_catalog* cat, int64_t B, const int64_t* rows, int32_t p,
                        int32_t c, void* workspace, size_t ws_bytes, int32_t* out_label,
                        int32_t* out_size, int32_t* out_medoid, int32_t* out_iters,
                        int32_t* status, void* stream);
int ebt_interest_interleave(const int32_t* size, const int64_t* list_rows,
                            const double* list_scores, int64_t B, int32_t c, int32_t k,
                            int64_t* out_rows, double* out_scores, int32_t* out_cluster,
                            int32_t* out_pos, void* stream);

/* ---- grouped top-k (0.12.0): the k best rows of every category from one scoring pass ---------
 * The reference keeps one list per user (lib.py:51-55); a front page shows a shelf per genre.
 * With allow masks alone that is G calls of the masked pipeline, each repeating the B x N
 * screening GEMM for the same query vectors. These entries score once and keep one list per
 * (query, group).
 *
 * The contract: for B queries and G mask ids groups[0..G) into ONE allow table (masks, words,
 * n_masks: the fields of ebt_allow above, bits indexed by GLOBAL row), the block
 * out[g][0..B)[0..k) of ebt_cosine_topk_grouped_prepared is bit for bit what
 * ebt_cosine_topk_prepared_allowed writes for the same operands with mask_id[b] = groups[g] for
 * every b, run unfused at the same chunk_rows and kprime: the same GLOBAL rows, float64 scores,
 * order (score descending, row ascending), NaN / -1 past the group's candidates, and the same
 * certificate in certified[g][b] (ebt_rescore's meaning: 1 exact, 0 widen k', -2 / -3 as there).
 * A row that belongs to several groups appears in each. groups[g] >= n_masks: an all-NaN / -1
 * shelf, nothing read out of bounds. groups[g] < 0: the unfiltered list. An id may occur twice.
 *
 * ebt_select_topk_grouped: the streaming select of ebt_select_topk (dense form) with one
 * candidate buffer and threshold per group in LDS. vals [B][ld] f32 (16-byte aligned,
 * ld % 4 == 0) holds the scores of GLOBAL rows [col_begin, col_begin + n); for each of `segs`
 * segments and each group the kprime largest entries whose bit is set in that group's mask,
 * sorted by (value descending, index ascending), go to
 * out_vals / out_idx[(g * B + b) * ld_out + seg * kprime + j] -- group-major, so that group g's
 * [B][kprime] block goes straight into ebt_rescore. out_idx holds GLOBAL rows. NaN and -inf
 * never enter; empty slots are -inf / -1, as ebt_select_topk's. One launch serves
 * ebt_grouped_pass_groups(kprime) groups (the largest count whose buffers fit the 64 KiB of LDS
 * the kernel asks for; >= 1 and non-increasing in kprime; 0 for a kprime out of range), so the
 * entry runs ceil(G / that) launches and EACH LAUNCH READS vals AGAIN. Found on the host before
 * any HIP call, EBT_EINVAL with a message that starts with the entry's name: a null pointer,
 * G outside [1, EBT_GROUPS_MAX], kprime outside [1, EBT_GROUPED_KPRIME_MAX], words not a
 * multiple of 4 or 32 * words < col_begin + n, n_masks < 1, ld % 4 != 0 or ld < n, B < 0,
 * n < 0, segs outside [1, 65535], ld_out < segs * kprime. B == 0 is EBT_OK without a launch.
 *
 * ebt_cosine_topk_grouped_prepared takes the 24 operands every prepared entry starts with, then
 * groups (device int32 [G]), G, the table, a workspace of ebt_cosine_topk_grouped_workspace(B,
 * B_pad, n_rows, kprime, chunk_rows, flags, G) bytes (EBT_ENOMEM when smaller; the sizing returns
 * 0 for arguments out of range), out_scores f64 [G][B][k], out_rows i64 [G][B][k], certified
 * i32 [G][B], timer, stream. It runs the unfused path only, one score chunk at a time
 * (ebt_screen_scores, or ebt_screen_exact under EBT_FLAG_EXACT; ebt_mask_excluded; the grouped
 * select), then one merge of every (g, b)'s per-chunk lists (ebt_select_topk's candidate-list
 * form over G B rows) and G rescores, one per group block. Timed under the existing stages
 * (EBT_STAGE_GEMM, _MASK, _SELECT, _MERGE_SELECT, _RESCORE): no new timer stage.
 * EBT_EUNSUPPORTED: min(k, n_rows) > EBT_GROUPED_KPRIME_MAX (the full-sort path included) and
 * row_offset != 0 (a row-sharded catalog). EBT_EINVAL as ebt_cosine_topk_prepared's, plus
 * kprime > EBT_GROUPED_KPRIME_MAX, G out of range and a bad table. */
#define EBT_GROUPS_MAX 64
#define EBT_GROUPED_KPRIME_MAX 512
int32_t ebt_grouped_pass_groups(int32_t kprime);
int ebt_select_topk_grouped(const float* vals, int64_t ld, int64_t B, int64_t n,
                            int64_t col_begin, const uint32_t* masks, int64_t words,
                            int32_t n_masks, const int32_t* groups, int32_t G, int32_t kprime,
                            int32_t segs, float* out_vals, int64_t* out_idx, int64_t ld_out,
                            void* stream);
size_t ebt_cosine_topk_grouped_workspace(int64_t B, int64_t B_pad, int64_t n_rows, int32_t kprime,
                                         int64_t chunk_rows, int flags, int32_t G);
int ebt_cosine_topk_grouped_prepared(
    const double* q64, const void* qimg, const float* qscale, const float* eps, int64_t B,
    int64_t B_pad, const void* cat, int dtype, int64_t ld, const double* gnorm64,
    const void* cimg, const float* cscale, int img_dtype, int32_t ld_img, int64_t n_rows,
    int32_t d, int32_t d_pad, int64_t row_offset, const int64_t* excl_off,
    const int64_t* excl_rows, int32_t k, int32_t kprime, int64_t chunk_rows, int flags,
    const int32_t* groups, int32_t G, const uint32_t* masks, int64_t words, int32_t n_masks,
    void* workspace, size_t ws_bytes, double* out_scores, int64_t* out_rows, int32_t* certified,
    void* timer, void* stream);

/* ---- two-phase top-k over a row-sharded catalog (robot_ebert_amd/distributed.py) ---------
 * Phase 1, every rank: ebt_cosine_screen = ebt_cosine_topk_prepared without the rescore: the shard's k'
 * best approx candidates, list_vals (f32) / list_rows (GLOBAL, -1 empty) [B][kprime]
 * partitioned at k as ebt_merge_hits describes (sorted when the unfused path ran),
 * ovf_out[b] = 1 when the fused screen overflowed for b, eps_out = the eps the certificate
 * must use. The ranks all-gather the lists and keep the k' best of all shards
 * (ebt_select_topk over [B][R*kprime] with the rows as indices).
 * Phase 2: ebt_rescore_owned writes the exact float64 score of every merged candidate whose
 * row is in [row_offset, row_offset + n_rows) and whose approx is >= approx[k-1] - 2 eps, 0.0
 * for the rest; an all-reduce (SUM) of `exact` completes it; ebt_finalize_topk sorts the
 * candidates above the cut by (exact desc, row asc) into out_scores/out_rows [B][k] and
 * certifies like ebt_rescore (ovf = the all-reduced (MAX) overflow flags -> certified -1; a
 * candidate row >= n_rows_global is no candidate and gives certified -2, which wins over -1). */
int ebt_cosine_screen(const double* q64, const void* qimg, const float* qscale, const float* eps,
                      int64_t B, int64_t B_pad, const void* cat, int dtype, int64_t ld,
                      const double* gnorm64, const void* cimg, const float* cscale, int img_dtype,
                      int32_t ld_img, int64_t n_rows, int32_t d, int32_t d_pad, int64_t row_offset,
                      const int64_t* excl_off, const int64_t* excl_rows, int32_t k, int32_t kprime,
                      int64_t chunk_rows, int flags, void* workspace, size_t ws_bytes,
                      float* list_vals, int64_t* list_rows, int32_t* ovf_out, float* eps_out,
                      void* timer, void* stream);
/* ---- shared screening threshold over a row-sharded catalog (distributed.py) -------------
 * The per-shard path (every rank: its exact top-k, then one all-gather + ebt_merge_topk)
 * screens every shard at ONE catalog-wide threshold instead of each shard's own:
 *   1. ebt_cosine_sample: `tiles` full 256-row tiles of this shard, `tile_stride` tiles apart
 *      from tile 0, through the screening GEMM keeping only the max of every 64-row subgroup:
 *      pooled[b * ld_pooled + 4 t + s] (B_pad rows, 4 * tiles maxima each; B_pad % 256 == 0).
 *   2. the ranks all-gather the maxima; ebt_pool_kth: theta[b] = the j-th largest of the G
 *      values pooled[b * ld + 0 .. G) (G <= 2048), -inf when fewer than j are >= -inf;
 *      theta[b] = +inf for B <= b < B_pad.
 *   3. ebt_cosine_screen_at = ebt_cosine_screen with the filter threshold theta[b] (device,
 *      [B]) instead of the shard's own sample estimate, `hits` = the expected hits per query on
 *      this shard (segment sizing). The list then holds this shard's rows with approx >= theta
 *      (and >= the list's own k-th - 2 eps once it has k rows): often fewer than k. Rows below
 *      theta are not screened out silently: theta is NOT checked here -- the caller must
 *      verify theta[b] <= t_floor[b] - eps[b] with the catalog-wide floor it passes to
 *      ebt_rescore, and rerun a query that fails (unfused, locally). kprime <= 512.
 * Replaces nothing in the reference (no sharding there). */
int ebt_cosine_sample(const void* qimg, const float* qscale, int64_t B_pad, const void* cimg,
                      const float* cscale, int img_dtype, int32_t ld_img, int64_t n_rows,
                      int32_t d_pad, int64_t tiles, int64_t tile_stride, float* pooled,
                      int64_t ld_pooled, void* timer, void* stream);
int ebt_pool_kth(const float* pooled, int64_t ld, int64_t B, int64_t B_pad, int32_t G, int32_t j,
                 float* theta, void* stream);
int ebt_cosine_screen_at(const double* q64, const void* qimg, const float* qscale,
                         const float* eps, int64_t B, int64_t B_pad, const void* cat, int dtype,
                         int64_t ld, const double* gnorm64, const void* cimg, const float* cscale,
                         int img_dtype, int32_t ld_img, int64_t n_rows, int32_t d, int32_t d_pad,
                         int64_t row_offset, const int64_t* excl_off, const int64_t* excl_rows,
                         int32_t k, int32_t kprime, int64_t chunk_rows, int flags,
                         void* workspace, size_t ws_bytes, float* list_vals, int64_t* list_rows,
                         int32_t* ovf_out, float* eps_out, const float* theta, double hits,
                         void* timer, void* stream);
/* The same two calls with a LEAD (0.3.1; lead = 0 is the calls above): the sample's first `lead`
 * tiles are the shard's first `lead` tiles (rows 0 .. 256 lead), the other tiles - lead follow
 * from tile `lead` on, `tile_stride` apart, and the lead tiles' scores are kept in
 * lead_scores[b * ld_lead + r] (ld_lead >= 256 lead). ebt_cosine_screen_at_lead takes the lead's
 * hits at theta from those scores and filters rows 256 lead .. n_rows only, so that the shard's
 * filter launches cover whole rounds of the persistent grid (driver.hip: the C ABI's sharded
 * step picks lead = ceil(n/256) mod (catalog tiles per round); 0 turns it off). */
int ebt_cosine_sample_lead(const void* qimg, const float* qscale, int64_t B_pad,
                           const void* cimg, const float* cscale, int img_dtype, int32_t ld_img,
                           int64_t n_rows, int32_t d_pad, int64_t tiles, int64_t tile_stride,
                           float* pooled, int64_t ld_pooled, int64_t lead, float* lead_scores,
                           int64_t ld_lead, void* timer, void* stream);
int ebt_cosine_screen_at_lead(const double* q64, const void* qimg, const float* qscale,
                              const float* eps, int64_t B, int64_t B_pad, const void* cat,
                              int dtype, int64_t ld, const double* gnorm64, const void* cimg,
                              const float* cscale, int img_dtype, int32_t ld_img, int64_t n_rows,
                              int32_t d, int32_t d_pad, int64_t row_offset,
                              const int64_t* excl_off, const int64_t* excl_rows, int32_t k,
                              int32_t kprime, int64_t chunk_rows, int flags, void* workspace,
                              size_t ws_bytes, float* list_vals, int64_t* list_rows,
                              int32_t* ovf_out, float* eps_out, const float* theta, double hits,
                              int64_t lead, const float* lead_scores, int64_t ld_lead,
                              void* timer, void* stream);
/* After the floor all-gather of the per-shard path: g = [R][B][ld] float32 (each shard's k best
 * approx in columns [0, ld-1), its eps in column ld-1) ->
 * t_floor[b] = the k-th largest of g[r][b][j] - g[r][b][ld-1] over all r and j < ld-1, in float64
 * (NaN counts as -inf): a lower bound of query b's k-th best exact score over the catalog. */
int ebt_union_floor(const float* gathered, int32_t R, int64_t B, int32_t ld, int32_t k,
                    double* t_floor, void* stream);
/* What a shard sends for that floor: out[b] = (the w largest of list_vals[b*ld + 0 .. n),
 * n = min(k_eff, ld), -inf padded to w; then eps[b], or -inf when eps is NULL) as [B][w + 1]
 * float32. The list may be
 * partitioned (any order): the w largest are selected. w = ebt_shard_list_width(k, world)
 * narrows the gather: the k-th largest over a subset of the shards' values is still a lower
 * bound, and with w >= a shard's share of the global top k it is the same bound. */
int ebt_floor_pack(const float* list_vals, int64_t ld, int64_t B, int32_t k_eff, int32_t w,
                   const float* eps, float* out, void* stream);
/* cert[b] = -1 (rerun unfused) where ovf[b] != 0, or where theta (if not NULL) may have dropped
 * a global top-k row: !(theta[b] <= t_floor[b] - eps[b]); a -2 (corrupt list) stays. */
int ebt_certify_cut(int32_t* cert, const int32_t* ovf, const float* theta,
                    const double* t_floor, const float* eps, int64_t B, void* stream);
int ebt_rescore_owned(const double* q64, int64_t B, int32_t d, const void* cat, int dtype,
                      int64_t ld, const double* gnorm64, int64_t row_offset, int64_t n_rows,
                      const float* cand_vals, const int64_t* cand_rows, int32_t kprime, int32_t k,
                      const float* eps, double* exact, void* stream);
int ebt_finalize_topk(const float* cand_vals, const int64_t* cand_rows, const double* exact,
                      int64_t B, int32_t kprime, int32_t k, int64_t n_rows_global,
                      const float* eps, const int32_t* ovf, double* out_scores, int64_t* out_rows,
                      int32_t* certified, void* stream);

/* ---- implicit-feedback ALS (offline factor training) ---------
 * Replaces pyspark.ml ALS(rank=32, maxIter=15, regParam=0.1, implicitPrefs=True) of
 * notebooks/create-embeddings.ipynb:1055 (Spark ALS.scala computeFactors, implicit branch).
 * ebt_als_gram: out[i*rank + j] = sum_r Y[r*rank + i] * Y[r*rank + j] (float64), Y n x rank f32.
 * ebt_als_solve: for every destination u (users from item factors Y, or items from user
 *   factors), with its ratings src[off[u] .. off[u+1]) / rating[...] (CSR):
 *     A = YtY + sum alpha|r| y y^T + reg * n_pos I,  b = sum_{r > 0} (1 + alpha|r|) y,
 *     X[u*rank ..] = (float) A^-1 b  (Cholesky in float64; n_pos = #ratings > 0).
 *   rank <= 64. */
int ebt_als_gram(const float* Y, int64_t n, int32_t rank, double* out, void* stream);
int ebt_als_solve(const double* YtY, const float* Y, int32_t rank, int64_t n_dst,
                  const int64_t* off, const int32_t* src, const float* rating, float alpha,
                  float reg, float* X, void* stream);

/* ---- per-stage GPU timing (hipEvents recorded on the launch stream) -----------------------
 * Stages: 0 screening GEMM (score-writing), 1 exclusion mask, 2 chunk select, 3 candidate
 * select (across chunks / head + fused tail), 4 rescore, 5 fused screening GEMM (filtering),
 * and the caller-bracketed stages of a row-sharded step: 6 query prep, 7 merge of the gathered
 * shard results, 8 stream stalls on collectives, 9 small per-batch kernels (thresholds, floors,
 * certificate checks).
 * ebt_timer_query synchronises the recorded events and returns the total milliseconds and the
 * number of launches of `stage` since the last reset. Host pointers.
 * ebt_timer_begin / ebt_timer_end bracket a caller's region of `stream` as one record of
 * `stage` (at most one open region per stage; nothing is recorded for a masked stage). */
#define EBT_STAGE_GEMM 0
#define EBT_STAGE_MASK 1
#define EBT_STAGE_SELECT 2
#define EBT_STAGE_MERGE_SELECT 3
#define EBT_STAGE_RESCORE 4
#define EBT_STAGE_GEMM_FILTER 5
#define EBT_STAGE_PREP 6
#define EBT_STAGE_SHARD_MERGE 7
#define EBT_STAGE_COLLECTIVE 8
#define EBT_STAGE_SMALL 9
#define EBT_NUM_STAGES 10
void* ebt_timer_create(void);
void ebt_timer_destroy(void* timer);
int ebt_timer_reset(void* timer);
/* Record only the stages whose bit (1 << EBT_STAGE_*) is set (default: all). */
int ebt_timer_set_mask(void* timer, uint32_t stage_mask);
int ebt_timer_query(void* timer, int stage, double* total_ms, int64_t* launches);
int ebt_timer_begin(void* timer, int stage, void* stream);
int ebt_timer_end(void* timer, int stage, void* stream);
/* Row accounting for the top-K roofline (bench.py `roofline_topk`): with on != 0 the timer owns
 * one device counter (allocated on the current device) to which every rescore kernel recorded
 * under EBT_STAGE_RESCORE on a stream of that device adds the candidate rows it gathered (one
 * atomic per query; launches on another device's streams are not counted, 0.3.2);
 * ebt_timer_reset zeroes it, ebt_timer_rows reads it (on the counter's device whatever device
 * is current; synchronise the launch streams first).
 * on = 0 frees it. Costs nothing when off. */
int ebt_timer_count_rows(void* timer, int on);
int ebt_timer_rows(void* timer, int64_t* rows);

#ifdef __cplusplus
}
#endif
#endif /* EBERT_H_ */
