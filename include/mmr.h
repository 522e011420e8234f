/* libmmr — MI355X (gfx950) joint-embedding retrieval hot path behind a C ABI.
 *
 * Every entry point takes plain pointers + sizes (no torch types), returns an mmr_status and, on
 * failure, leaves a message in the thread-local mmr_last_error().  No exceptions cross the ABI.
 * Ownership: the caller owns every input/output buffer (device pointers unless a parameter says
 * host); the library owns mmr_index state and its workspaces.  Launches are asynchronous on the
 * caller's HIP stream (`stream` = hipStream_t, NULL = default stream).
 *
 * Reference interfaces replaced (file:line in ppddddpp/multi-modal-retrieval-predict-project):
 *   mmr_index_create   RetrievalEngine.__init__  src/Retrieval/retrieval.py:24-32
 *                      (np.load(...).astype(float32) -> self.embs (N,D)); norms precomputed once
 *                      instead of sklearn normalize() per call (retrieval.py:128).
 *   mmr_index_search   exact brute-force top-K: sklearn cosine_similarity + np.argsort(...)[::-1][:K]
 *                      src/Evaluate/retrieval_overlap.py:84-90, src/Retrieval/retrieval.py:128-137;
 *                      reached via RetrievalEngine.retrieve retrieval.py:34-39.
 *   mmr_merge_topk     (new) k-way merge of per-shard top-K lists after the RCCL all-gather.
 *   tower ops          timm SwinTransformer.forward_features (src/Model/fusion.py:198-199),
 *                      HF BertModel(...).last_hidden_state (fusion.py:322-325), heads
 *                      src/Model/model.py:365-373,462-479; see the per-function comments.
 */
#ifndef MMR_H
#define MMR_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  MMR_OK = 0,
  MMR_ERR_INVALID = 1,     /* bad argument (shape, null pointer, unsupported K/D) */
  MMR_ERR_HIP = 2,         /* a HIP runtime call failed */
  MMR_ERR_OOM = 3,         /* device allocation failed */
  MMR_ERR_UNSUPPORTED = 4, /* dtype / geometry not built */
  MMR_ERR_CAPACITY = 5     /* a per-query candidate buffer overflowed (see out_status) */
} mmr_status;

typedef enum { MMR_F32 = 0, MMR_F16 = 1, MMR_BF16 = 2 } mmr_dtype;

typedef struct mmr_index mmr_index;

const char* mmr_last_error(void);
int mmr_version(void);
int mmr_max_k(void);

/* ---------------------------------------------------------------- gallery index (kNN) */
/* Copy an (n, d) row-major gallery (host pointer if `gallery_is_host`, else device) into a
 * library-owned device layout on `device`, computing per-row inverse norms (f32) and norms (f64).
 * `idx_base` is added to every returned index (row-sharded galleries: global = local + base).
 * dtype MMR_F32: f32 rows (every scan mode).  MMR_F16: a native fp16 index — the raw fp16 rows are its only
 * device copy (2 B per element + f32 inverse norms + f64 norms per row), scanned in mode 2 only (its exact
 * f64 re-score reads the same rows: fp16 is exact in f64), results bit-identical to an MMR_F32 index of the
 * f32-upcast rows; mmr_index_set_mode(0 / 1) returns MMR_ERR_UNSUPPORTED.  MMR_BF16: not built. */
mmr_status mmr_index_create(const void* gallery, int64_t n, int32_t d, mmr_dtype dtype,
                            int gallery_is_host, int64_t idx_base, int device, mmr_index** out);
mmr_status mmr_index_destroy(mmr_index* index);
mmr_status mmr_index_info(const mmr_index* index, int64_t* n, int32_t* d, int64_t* idx_base);
/* Device bytes the index holds: gallery_bytes = the rows + norms + the scan copies of the current mode.
 * MMR_F32 index: f32 rows (4 B per element) + the current mode's copies (x3: bf16 hi/lo split + tile16 f32,
 * 8 B per element; f16: ONE fp16 unit-row copy in the tile32h layout, 2 B per element; f32: none — copies
 * of other modes are freed at a mode switch).  MMR_F16 index: the fp16 rows only (2 B per element).
 * workspace_bytes = the query / per-unit-maxima workspace.  Either pointer may be NULL. */
mmr_status mmr_index_device_bytes(const mmr_index* index, int64_t* gallery_bytes, int64_t* workspace_bytes);
/* Pre-allocate the workspace for up to `max_q` queries in the CURRENT scan mode so that later
 * searches allocate nothing (required before capturing a search into a HIP graph). */
mmr_status mmr_index_reserve(mmr_index* index, int64_t max_q);

/* Scan precision of the candidate pass (the ranking is always exact f64): 0 = f32 MFMA,
 * 1 = bf16 3-term split MFMA (default; ~5x the f32 rate at the same bytes; queries chunks of
 * <= 32 take the HBM-streaming f32 skinny scan), 2 = fp16 unit-row copy of the gallery (built on
 * the first switch to this mode: half the scan bytes, one fp16 MFMA per product, a wider candidate
 * margin — the same exact results). */
mmr_status mmr_index_set_mode(mmr_index* index, int32_t mode);

/* Exact cosine top-K of q (q, d) f32 device queries against the gallery.
 * Semantics: s(q,g) = <q,g> / (|q| |g|) in f64 (0 when either norm is 0 — sklearn's normalize()
 * leaves zero rows at 0), ranked by score descending, ties by lower gallery index.  Outputs
 * (q, k) int64 indices (+idx_base) and f32 scores; slots beyond n are (-1, -inf).
 * out_status (q,) int32 (may be NULL): per-query status, always 0 — more candidates inside the scan
 * margin than the selection buffer holds (massive near-ties) are merged batch by batch inside the
 * selection kernel, exactly, never truncated (a non-zero value would flag an inexact list).
 * Asynchronous on `stream`.  Threading: calls on one index may come from several host threads and
 * several streams; the index's workspace follows the stream (a search on a new stream first waits
 * for the previous search's last use), so concurrent searches serialise on the device but never race.
 * The hand-over event is recorded on the previous search's stream at the switch (not after every
 * search: a per-search event record cost 3-5 us of device time), so that stream must still exist
 * when a search on another stream, or a workspace growth, follows. */
mmr_status mmr_index_search(mmr_index* index, const float* q, int64_t nq, int32_t k,
                            int64_t* out_idx, float* out_score, double* out_score64,
                            int32_t* out_status, void* stream);
/* out_score64 (q, k) f64 (may be NULL): the exact scores the ranking used; the shard merge ranks
 * on these so a row-sharded search returns exactly the single-device result. */

/* DLS link graph (DLSRetrievalEngine._build_link_graph, src/Retrieval/retrieval.py:121-138): the
 * self-join of gallery rows [row0, row0+nrows) against the whole index — per row its neighbours
 * in exact-cosine order (score desc, index asc), the row itself excluded (the reference's diagonal
 * -1), score >= threshold, at most max_links.  out_nbr (nrows, max_links) int64 LOCAL row indices,
 * -1 padded; out_cnt (nrows,) int32.  Device buffers, asynchronous on `stream`. */
mmr_status mmr_index_link_graph(mmr_index* index, double threshold, int32_t max_links, int64_t row0,
                                 int64_t nrows, int64_t* out_nbr, int32_t* out_cnt, void* stream);

/* Batched DLS walk (DLSRetrievalEngine.retrieve without reranking, src/Retrieval/retrieval.py:198-244): nq
 * independent greedy walks over a link graph of this index, one wavefront per query.  The reference's heap only
 * holds a totally ordered set, so the walk is stated, and implemented, as a set algorithm:
 *   score(i) = <g_i, q> / fma(|g_i|, |q| + 1e-6, 1e-12) in f64 (the denominator is ONE fused multiply-add): the
 *     reference's expression, not mmr_index_search's cosine.  <g_i, q> is summed in f64 from the f32 row and query
 *     in one fixed order (lane l of 64 takes the floats 256 c + 4 l .. + 3 of every 256-float chunk c in ascending
 *     order, f64 FMAs; the 64 partials through the xor 32, 16, 8, 4, 2, 1 tree), |g_i| is the index's f64 row norm,
 *     |q| the square root of the same tree's sum of the lanes' q^2 partials.  The score of a row depends on nothing
 *     but the row and the query: not on the batch slot, the neighbour position or the rows loaded with it, so
 *     byte-identical rows tie bit for bit.  A zero row or a zero query scores 0.
 *   order: score descending, then LOCAL row index ascending ("best" below).
 *   set, visited := the seeds; a seed or neighbour that is < 0, >= n or already visited is skipped (-1 padding,
 *     garbage, self-loops, a row listed twice).
 *   while steps < max_steps and the set is not empty: remove the best row b from the set; add every unvisited
 *     nbr[b][0 .. max_links) to visited and to the set; if the set holds more than r rows keep the best r; if no
 *     row was added the walk stops (that step is not counted, b stays removed); else steps += 1.
 *   output: the best min(k, |set|) rows, written in (score descending, index DESCENDING) order — the reference's
 *     sorted(..., reverse=True) over (sim, idx) tuples: a run of equal scores that straddles the k boundary keeps
 *     its lower indices and prints them high to low.  Slots past the set are (-1, -inf).
 * q (nq, d) f32; nbr (n, max_links) int64 LOCAL rows as mmr_index_link_graph writes them; seeds (nq, seed_size)
 * int64 LOCAL rows; r = the reference's R = max(candidate_multiplier * K, seed_size).  out_idx (nq, k) int64
 * GLOBAL (+ idx_base), out_score (nq, k) f32, out_score64 (nq, k) f64 (may be NULL), out_steps / out_visited (nq)
 * int32 (may be NULL): the counted steps and |visited|.
 * Limits (MMR_ERR_INVALID beyond them, before any launch): 1 <= r <= 512; 1 <= max_links <= 32; 1 <= k <= r;
 * 0 <= seed_size <= r; max_steps >= 0; min(n, seed_size + max_steps * max_links) <= 4096 (the visited set; the
 * reference's defaults at max_links = 32 need 3205); d <= 1024; n < 2^31; nq < 2^31.  An MMR_F32 index only: a
 * native fp16 index returns MMR_ERR_UNSUPPORTED.  All pointers device; asynchronous on `stream`, no host
 * synchronisation, no allocation (the working sets live in LDS), no atomics on global memory: two runs give
 * identical bytes.  nq == 0 launches nothing. */
mmr_status mmr_index_dls_walk(const mmr_index* index, const float* q, int64_t nq, const int64_t* nbr,
                              int32_t max_links, const int64_t* seeds, int32_t seed_size, int32_t k,
                              int32_t max_steps, int32_t r, int64_t* out_idx, float* out_score,
                              double* out_score64, int32_t* out_steps, int32_t* out_visited, void* stream);

/* KG / label reranker fused after the top-K (Reranker.rerank, src/Retrieval/reranker.py:240-333):
 * per query the kc candidates cand (nq, kc) int64 (global indices into this index, -1 = empty,
 * kc <= 64) are re-scored with alpha*minmax(cos(q_emb, row)) + beta*minmax(Jaccard(label sets)) +
 * gamma*minmax(cos(kg vectors)) — cosines in f64, 0 for a zero norm — and the first topk written
 * in final-score order (equal finals: later candidate first, as np.argsort(final)[::-1]).
 * q_emb (nq, d) f32; q_labels (nq) / g_labels (n) uint64 label bitsets; q_kg (nq, dk) /
 * g_kg (n, dk) f32 record KG vectors (g_* in local row order).  Outputs (nq, topk): out_idx int64,
 * optional out_final / out_emb / out_lab / out_kg f64 (the scaled components, like the reference's
 * result tuples).  A candidate is valid when it is >= 0 and a row of this index ([idx_base,
 * idx_base + n)); the min-max runs over the valid candidates only, and every output slot past their
 * number is written: out_idx -1, the f64 outputs 0.0. */
mmr_status mmr_index_rerank(const mmr_index* index, const float* q_emb, int64_t nq, const int64_t* cand,
                            int32_t kc, const uint64_t* q_labels, const uint64_t* g_labels, const float* q_kg,
                            const float* g_kg, int32_t dk, double alpha, double beta, double gamma,
                            int32_t topk, int64_t* out_idx, double* out_final, double* out_emb,
                            double* out_lab, double* out_kg, void* stream);

/* Merge n_lists per-shard lists laid out [n_lists][nq][k_in] (f64 scores, int64 idx; empty slots
 * idx -1, anywhere in a list, their scores ignored) into the global top-k_out per query: score desc,
 * then index asc, then source position (list, slot) asc — an entry that two lists deliver with the
 * same score and index is kept twice, in source order, each with its own payload.  Slots past the
 * valid entries are (-1, -inf, zero payload).  n_lists * k_in <= 4096.  out_score f32 (may be NULL),
 * out_score64 f64 (may be NULL). */
mmr_status mmr_merge_topk(const double* scores, const int64_t* idx, int32_t n_lists, int64_t nq,
                          int32_t k_in, int32_t k_out, int64_t* out_idx, float* out_score,
                          double* out_score64, void* stream);
/* mmr_merge_topk over queries [q0, q0 + nq) of lists laid out [n_lists][nq_total][k_in] (a rank
 * merges only its own queries after the all-gather), with an optional f64 payload of
 * payload_width (<= 16) values per entry, [n_lists][nq_total][k_in][width], carried into
 * out_payload [nq][k_out][width] (zeros for empty slots).  payload and out_payload are both NULL or
 * both set.  The sharded rerank's per-candidate components ride here (reranker.py:240-333 needs
 * them over the MERGED candidate list). */
mmr_status mmr_merge_topk_payload(const double* scores, const int64_t* idx, const double* payload,
                                  int32_t payload_width, int32_t n_lists, int64_t nq_total, int64_t q0,
                                  int64_t nq, int32_t k_in, int32_t k_out, int64_t* out_idx, float* out_score,
                                  double* out_score64, double* out_payload, void* stream);

/* mmr_merge_topk_payload over ONE packed all-gather buffer (the sharded search's single collective,
 * SURVEY.md §8e): packed = [n_lists][nq_total][k_in][2 + payload_width] 8-byte words per entry =
 * {f64 score, int64 global index (-1 = empty), payload_width f64 payload values}; merges queries
 * [q0, q0 + nq) (score desc, index asc) into out_idx / out_score / out_score64 / out_payload
 * [nq][k_out][payload_width] (each output but out_idx may be NULL). */
mmr_status mmr_merge_topk_packed(const void* packed, int32_t payload_width, int32_t n_lists, int64_t nq_total,
                                 int64_t q0, int64_t nq, int32_t k_in, int32_t k_out, int64_t* out_idx,
                                 float* out_score, double* out_score64, double* out_payload, void* stream);

/* Sharded KG / label rerank (Reranker.rerank, src/Retrieval/reranker.py:240-333, over a row-sharded
 * gallery).  Shard side: mmr_index_rerank_components writes, for each of this shard's candidates
 * cand (nq, kc) (global indices into this index, -1 = empty), the three RAW components
 * out_comp (nq, kc, 3) f64 = {emb cosine, label Jaccard, KG cosine} — the same f64 arithmetic as
 * mmr_index_rerank (zeros for an empty slot).  They travel with the (score, index) lists through
 * the all-gather and mmr_merge_topk_payload; mmr_rerank_mix then min-max scales them over the
 * merged list, mixes alpha/beta/gamma and ranks exactly as mmr_index_rerank does, so a sharded
 * rerank returns bit-identical results to the single-index one.  Arguments as mmr_index_rerank. */
mmr_status mmr_index_rerank_components(const mmr_index* index, const float* q_emb, int64_t nq,
                                       const int64_t* cand, int32_t kc, const uint64_t* q_labels,
                                       const uint64_t* g_labels, const float* q_kg, const float* g_kg,
                                       int32_t dk, double* out_comp, void* stream);
mmr_status mmr_rerank_mix(const int64_t* cand, const double* comp, int64_t nq, int32_t kc, double alpha,
                          double beta, double gamma, int32_t topk, int64_t* out_idx, double* out_final,
                          double* out_emb, double* out_lab, double* out_kg, void* stream);

/* Full-ranking label evaluation (compute_ranking_metrics, src/Evaluate/retrieval_overlap.py:84-115; the
 * test -> test ground truth of contructGT.py:73 drops the query itself): the rank of the first gallery row that
 * shares a label with the query, over the WHOLE gallery, and the number of such rows.  For query q and row g:
 *   score(q, g) = <q, g> / (|q| |g|) in f64 of the raw rows (fp16 rows upcast exactly), 0 when either norm is 0
 *     — mmr_index_search's expression.  The contraction runs on the f64 matrix unit in a summation order of its
 *     own, so a score may differ from mmr_index_search's out_score64 in the last bits; what holds instead: the
 *     order is the same for every (query, row) pair, for both index dtypes and in both entry points, so
 *     byte-identical rows score bit-identically and mmr_index_count_ahead reproduces the score
 *     mmr_index_best_relevant returned for a row bit for bit.
 *   order: score descending, then GLOBAL index (idx_base + row) ascending — the search's order.
 *   g is relevant iff (g_labels[g] & q_labels[q]) != 0.
 *   g is excluded iff exclude != NULL && exclude[q] == the global index of g (exclude[q] < 0: nothing): an
 *     excluded row is neither relevant nor counted ahead of anything.
 *   Only rows < n exist: the padding of the device layout is masked by row number, never by score.
 * mmr_index_best_relevant: per query the first relevant row under the order — out_idx (nq) global index, -1 when
 *   there is none; out_score (nq, may be NULL) its score, 0.0 when none — and out_nrel (nq, may be NULL) the number
 *   of relevant rows.  q (nq, d) f32; q_labels (nq) / g_labels (n, this index's rows in local order) uint64 bitsets.
 * mmr_index_count_ahead: per query the number of this index's existing, non-excluded rows ranked strictly ahead of
 *   (ref_score, ref_idx): score > ref_score, or score == ref_score and global index < ref_idx.  ref_idx is a global
 *   index and need not be a row of this index (row-sharded galleries: every shard counts against the global best
 *   and the counts add up); ref_idx[q] < 0: out_ahead[q] = 0 and no work for that query.
 *   first_rank = 1 + count_ahead(best_relevant), 0 when there is no relevant row.
 * work: mmr_index_rank_work_bytes(index, nq) bytes of scratch owned by the caller, 16-B aligned (the index is
 *   const: neither call touches its search workspace).  Any nq (queries run in internal passes); nq == 0 launches
 *   nothing.  All pointers device, asynchronous on `stream`.  No atomics: two runs give identical bytes. */
int64_t mmr_index_rank_work_bytes(const mmr_index* index, int64_t nq);
mmr_status mmr_index_best_relevant(const mmr_index* index, const float* q, int64_t nq, const uint64_t* q_labels,
                                   const uint64_t* g_labels, const int64_t* exclude, int64_t* out_idx,
                                   double* out_score, int64_t* out_nrel, void* work, void* stream);
mmr_status mmr_index_count_ahead(const mmr_index* index, const float* q, int64_t nq, const int64_t* ref_idx,
                                 const double* ref_score, const int64_t* exclude, int64_t* out_ahead, void* work,
                                 void* stream);

/* Retrieval diversity of retrieved lists (compute_embedding_diversity / compute_label_diversity_from_labels,
 * src/Evaluate/retrieval_diversity_compute.py:171-194), for nq lists at once.  idx (nq, k) int64 holds GLOBAL
 * indices as mmr_index_search, mmr_index_dls_walk and mmr_index_rerank write them.  For one list idx[q][0 .. k):
 *   valid: an entry is valid iff idx_base <= idx < idx_base + n; every other entry is skipped (the -1 padding of
 *     walks and short galleries, garbage: the reference's `if r in id_to_emb`).  m = the number of valid entries.
 *     A row listed twice counts twice; its pair with itself elsewhere in the list is an ordinary pair.
 *   cosine: c(i, j) = <g_i, g_j> / (max(|g_i|, 1e-8) * max(|g_j|, 1e-8)) in f64 of the raw rows (fp16 rows upcast
 *     exactly), |g| = the index's f64 row norm.  The 1e-8 clip is the reference's norms.clip(min=1e-8), NOT
 *     mmr_index_search's "0 when a norm is 0": a zero row gives 0 either way, a row whose norm is below 1e-8 gives a
 *     shrunken, nonzero cosine (two rows of 1e-9 at d = 4: diversity 0.96).
 *   out_emb[q] = (m < 2) ? 0.0 : 1 - (sum over valid list positions i < j of c(i, j)) / (m (m - 1) / 2).  The sum
 *     runs in one fixed order that depends on the list's own contents and k only — never on nq, the batch slot or
 *     neighbouring lists (csrc/list_div.hip states it).  No atomics: two runs give identical bytes.
 *   labels (g_labels (n) uint64 bitsets in local row order, as mmr_index_rerank's): over the valid entries
 *     u = popcount(OR of the bitsets), s = sum of the popcounts, c = the number of entries with a non-empty bitset;
 *     out_lab[q] = (c == 0) ? 0.0 : (double)u / ((double)s / (double)c) — two f64 divisions in this order,
 *     contraction off: the reference's len(all_labels) / float(np.mean(sizes_nonzero)) bit for bit.
 *     g_labels and out_lab are both NULL or both set.
 *   out_valid (nq) int32 = m; may be NULL.
 *   out_sim (nq, k, k) f64, may be NULL: c(i, j) at the list positions, the diagonal included, from the same
 *     expression; every row and column of an invalid entry is 0.0; (i, j) and (j, i) hold the same bits.
 * Limits (MMR_ERR_INVALID beyond them, before any launch): 1 <= k <= mmr_max_k() (256); nq >= 0 (nq == 0 launches
 * nothing); idx and out_emb non-NULL.  Both index kinds (MMR_F32, MMR_F16).  work:
 * mmr_index_list_diversity_work_bytes(index, nq, k) bytes of scratch owned by the caller, 16-B aligned (0 bytes,
 * and work may be NULL, for k <= 16: one wavefront finishes such a list; beyond, per-tile-pair partial sums pass
 * through it).  The index is const: its search workspace is not touched.  All pointers device, asynchronous on
 * `stream`, no host synchronisation, no allocation. */
int64_t mmr_index_list_diversity_work_bytes(const mmr_index* index, int64_t nq, int32_t k);
mmr_status mmr_index_list_diversity(const mmr_index* index, const int64_t* idx, int64_t nq, int32_t k,
                                    const uint64_t* g_labels, double* out_emb, double* out_lab, int32_t* out_valid,
                                    double* out_sim, void* work, void* stream);

/* ---------------------------------------------------------------- tower ops (bf16 = uint16) */
/* Y[m][n] = act(X[m][k] . W[n][k]^T + bias[n]) (+ R[m][n]); X, W, R, Y bf16; bias f32 or NULL;
 * act: 0 none, 1 GELU(erf).  nn.Linear semantics (weight [out][in]).  f32 accumulation. */
mmr_status mmr_linear_bf16(const uint16_t* x, const uint16_t* w, const float* bias,
                           const uint16_t* residual, uint16_t* y, int64_t m, int32_t n, int32_t k,
                           int32_t act, void* stream);

/* The launch variant mmr_linear_bf16 settled on for this shape / epilogue on the current device
 * (the first call per shape times the variants and keeps the fastest), or -1 before that call.
 * Diagnostic: lets a benchmark name the kernel it measured. */
int32_t mmr_linear_bf16_variant(int64_t m, int32_t n, int32_t k, int32_t act, int32_t has_bias,
                                int32_t has_residual);
/* The BERT linears with the residual LayerNorm folded in, so no LayerNorm pass runs between the
 * GEMMs of a layer (HF BertLayer: LN(dense(x) + residual), reference fusion.py:322-325 via BertModel).
 * Persistent 8-phase bf16 GEMM, 256-row tiles: m % 256 == 0, k % 128 == 0, n % 192 == 0 or n % 256 == 0.
 *   stats_out (optional, act == 0): per row, parts = mmr_linear_bf16_ln_parts(m, n, ln_mode) f32 pairs
 *     (sum, M2) of the bf16 outputs as stored — [m][parts][2]: part p covers the n / parts columns
 *     [p n / parts, (p + 1) n / parts) and M2 is its CENTRED sum of squares, sum (y - part mean)^2 (not
 *     a raw sum of squares); mmr_ln_row_coef merges the parts with Chan's parallel formula into the
 *     row's LayerNorm statistics (deterministic: one pair per tile column and wave column, no atomics).
 *   ln_mode 0: y = act(x W^T + bias) (+ residual).
 *   ln_mode 1: x is a raw residual-stream row y_in produced with stats, ln_coef = its mmr_ln_row_coef
 *     (f32 [m][2]); w = W diag(gamma) (bf16), ln_v1 = c = row sums of w (f32 [n]),
 *     bias = W beta + b:  y = act(LN(y_in) W^T + b) = act(rstd (y_in w^T) - rstd mean c + bias).
 *   ln_mode 2: residual is a raw row r produced with stats, ln_coef its coefficients; ln_v1 / ln_v2 =
 *     gamma / beta (f32 [n]):
 *     y = x W^T + bias + LN(r)  (n % 192 == 0).
 * Built: mode 1 with or without GELU (no residual, no stats); mode 2 with or without stats; mode 0
 * with stats, with or without a residual.  bias is required.  MMR_ERR_UNSUPPORTED otherwise. */
mmr_status mmr_linear_bf16_ln(const uint16_t* x, const uint16_t* w, const float* bias,
                              const uint16_t* residual, uint16_t* y, int64_t m, int32_t n, int32_t k,
                              int32_t act, int32_t ln_mode, const float* ln_coef, const float* ln_v1,
                              const float* ln_v2, float* stats_out, void* stream);

/* The row statistics of a producer (stats [m][nparts][2] = per part (sum, centred M2) over n / nparts
 * columns each, as mmr_linear_bf16_ln writes them; nparts even, n % nparts == 0 — checked) -> LayerNorm
 * coefficients coef [m][2] = (rstd, -mean rstd) over the row width n, rstd = 1 / sqrt(var + eps):
 * mean = sum_p sum_p / n, M2 = sum_p M2_p + (n / nparts) sum_p (mean_p - mean)^2 (Chan). */
mmr_status mmr_ln_row_coef(const float* stats, int64_t m, int32_t nparts, int32_t n, float eps, float* coef,
                           void* stream);

/* Row-statistics pairs per row mmr_linear_bf16_ln writes for an m x n output in ln_mode (0: not built). */
int32_t mmr_linear_bf16_ln_parts(int64_t m, int32_t n, int32_t ln_mode);

/* Number of launch variants mmr_linear_bf16 chooses among (indices 0 .. n-1 of its table). */
int32_t mmr_linear_bf16_n_variants(void);

/* The kernels mmr_linear_bf16 launches (its routes).  A variant names a wish; the shape guards decide (DESIGN.md,
 * "Routes of the bf16 tiled GEMM"): a variant whose guards fail falls through to a later route, at last to BASE.
 * Residual rounding: the BASE and BIG routes round act(acc + bias) to bf16 and round again after adding the bf16
 * residual (two roundings); the P8 routes add the residual in f32 and round once; the W4 routes take no residual. */
enum {
  MMR_GEMM_ROUTE_BASE_128X128 = 0,       /* gemm_bf16_tn: 4 waves, any m; n, k multiples of 8 */
  MMR_GEMM_ROUTE_W4_256X256 = 1,         /* gemm_bf16_tn_w4<8>: persistent, 4 waves, no residual */
  MMR_GEMM_ROUTE_W4_256X192 = 2,         /* gemm_bf16_tn_w4<6> */
  MMR_GEMM_ROUTE_BIG_256X256_KB64X2 = 3, /* gemm_bf16_tn_big, 8 waves: tile, K slice depth x LDS stages */
  MMR_GEMM_ROUTE_BIG_256X256_KB32X4 = 4,
  MMR_GEMM_ROUTE_BIG_256X192_KB64X2 = 5,
  MMR_GEMM_ROUTE_BIG_256X128_KB32X2 = 6,
  MMR_GEMM_ROUTE_BIG_256X128_KB32X3 = 7,
  MMR_GEMM_ROUTE_BIG_256X128_KB64X3 = 8,
  MMR_GEMM_ROUTE_P8_256X256 = 9,         /* gemm_bf16_tn_p8<4>: persistent 8-phase, 8 waves */
  MMR_GEMM_ROUTE_P8_256X192 = 10,        /* gemm_bf16_tn_p8<3> */
  MMR_GEMM_N_ROUTES = 11
};
/* The kernel mmr_linear_bf16 launches for (m, n, k, has_residual) under `variant` on a device with `cus`
   compute units (cus <= 0: the current device).  Launches nothing.  -1: bad arguments (what mmr_linear_bf16
   refuses, m = 0, or a variant outside 0 .. mmr_linear_bf16_n_variants() - 1). */
int32_t mmr_linear_bf16_route(int64_t m, int32_t n, int32_t k, int32_t has_residual, int32_t variant, int32_t cus);

/* Test / A-B hook (the product path never calls it): pin a launch variant for the whole process.
 *   MMR_PIN_GEMM_BF16: value = mmr_linear_bf16 variant index, or -1 = per-shape tuning (default);
 *   MMR_PIN_X3_WAVES:  value = 4 or 8 waves per mmr_linear_x3 tile (8 only where K % 256 == 0),
 *                      or -1 = automatic (default).
 *   MMR_PIN_X3_MLP:    value = 0 (8-wave workgroups) or 1 (4-wave workgroups, two per CU) for
 *                      mmr_x3_swin_mlp at C = 96, or -1 = automatic (1).  Both give bit-identical outputs.
 *   MMR_PIN_SWA:       route of mmr_swin_window_attention: 0 = the gather kernel, 1 = the streaming kernel
 *                      wherever it takes the geometry (7 x 7 windows, an even number of heads; any other
 *                      geometry, and the _q8 form, stay on the gather kernel), -1 = automatic (default: the
 *                      streaming kernel from 3 units per wave up).  Both give bit-identical outputs.
 *                      Launch rule of the streaming kernel: units = b * (hw / 7)^2 * (heads / 2), ordered
 *                      (window, head pair)-major with the images innermost; workgroups of 4 waves,
 *                      min(CUs, ceil(units / 4)) of them; wave g of the G = 4 * workgroups takes the units
 *                      [g * units / G, (g + 1) * units / G) (integer division).
 * MMR_ERR_INVALID for an unknown pin or value. */
enum { MMR_PIN_GEMM_BF16 = 0, MMR_PIN_X3_WAVES = 1, MMR_PIN_X3_MLP = 2, MMR_PIN_SWA = 3 };
mmr_status mmr_pin_variant(int32_t which, int32_t value);

/* Resident-weight streaming linear for the short-K, narrow tower linears (Swin patch embed, stage-2
 * qkv / proj, PatchMerging 1->2; timm nn.Linear, reference fusion.py:198-199):
 * y = x @ W^T + bias (+ residual), K in {64, 192}.  W is kept in LDS for the whole launch, as
 * mmr_linear_rw_parts(n, k) parts of N / P channels, from an image built once by
 * mmr_linear_rw_pack (n * k bf16 elements, caller-allocated).  mmr_linear_rw_parts returns 0 for
 * shapes it does not take (then use mmr_linear_bf16). */
int32_t mmr_linear_rw_parts(int32_t n, int32_t k);
mmr_status mmr_linear_rw_pack(const uint16_t* w, int32_t n, int32_t k, uint16_t* img, void* stream);
mmr_status mmr_linear_rw(const uint16_t* x, const uint16_t* img, const float* bias, const uint16_t* residual,
                         uint16_t* y, int64_t m, int32_t n, int32_t k, void* stream);

/* Per-query f32 linears on bf16x3 MFMA (the multimodal head's per-vector chain, reference model.py:375-459):
 * y = act(x @ W^T + bias) (+ residual), x / y / residual f32 rows (strides ldx / ldy / ldr), W given as its
 * bf16 split W_hi = bf16(W), W_lo = bf16(W - W_hi) ([cout][cin] each); x is split the same way in
 * registers and each product summed as hi*hi + hi*lo + lo*hi in f32 (~2^-17 relative per product).
 * nbatch independent problems at element strides bsx / bsw / bsb / bsr / bsy (nbatch = 1: one linear).
 * cin % 128 == 0, cout % 32 == 0; residual may alias y. */
mmr_status mmr_linear_x3(const float* x, int64_t ldx, int64_t bsx, const uint16_t* w_hi, const uint16_t* w_lo,
                         int64_t bsw, const float* bias, int64_t bsb, const float* residual, int64_t ldr, int64_t bsr,
                         float* y, int64_t ldy, int64_t bsy, int32_t nbatch, int32_t b, int32_t cin, int32_t cout,
                         int32_t act, void* stream);

/* ---------------------------------------------------------------- MX-fp8 linears (config 5) */
/* Quantise bf16 x [rows][k] to OCP e4m3 q [rows][kp] (zero-padded, kp >= k, kp % 256 == 0) with one
 * E8M0 scale per 32 consecutive k of a row: 2^e, the smallest e with amax <= 448 * 2^e (no clipping);
 * q = RNE(x * 2^-e).  The scale bytes are written in the GEMM's per-lane LDS image order:
 * layout 0 (activations, rows % 256 == 0): [rows/256][kp/128][2][4][16][8] (1 byte per row-block);
 * layouts 1 / 2 (weights, rows % 192 / 256 == 0, for 256 x 192 / 256 x 256 GEMM tiles):
 * [rows/PR][kp/128][4][4][16][4] = rows/PR * kp/128 * 1024 bytes (PR = 192 / 256).  Replaces the bf16 operand of the Swin / BERT nn.Linear (fusion.py:198-199, 322-325) on the
 * fp8 tower path. */
mmr_status mmr_quantize_mxfp8(const uint16_t* x, int64_t rows, int32_t k, int32_t kp, int32_t layout,
                              uint8_t* q, uint8_t* scales, void* stream);

/* Y[m][n] = act(dequant(Xq) . dequant(Wq)^T + bias[n]) (+ R[m][n]) with gfx950 block-scaled MFMA
 * (v_mfma_scale_f32_16x16x128_f8f6f4, e4m3 x e4m3, f32 accumulation); Xq/xs from layout 0, Wq/ws
 * from layout w_layout (1 or 2) of mmr_quantize_mxfp8; Y, R bf16.  m % 256 == 0, kp % 256 == 0,
 * n % 192 == 0 (w_layout 1) or n % 256 == 0 (w_layout 2). */
mmr_status mmr_linear_mxfp8(const uint8_t* xq, const uint8_t* xs, const uint8_t* wq, const uint8_t* ws,
                            int32_t w_layout, const float* bias, const uint16_t* residual, uint16_t* y,
                            int64_t m, int32_t n, int32_t kp, int32_t act, void* stream);

/* mmr_linear_mxfp8 (weights in layout 2, no residual) whose output is written directly as the next
 * GEMM's MX-fp8 activation operand: yq [m][n] e4m3 + ys layout-0 scales (m/256 * n/128 * 1024 bytes),
 * bit-identical to mmr_quantize_mxfp8 of the bf16 output (BERT FFN1 -> FFN2, Swin fc1 -> fc2). */
mmr_status mmr_linear_mxfp8_q8(const uint8_t* xq, const uint8_t* xs, const uint8_t* wq, const uint8_t* ws,
                               const float* bias, uint8_t* yq, uint8_t* ys, int64_t m, int32_t n,
                               int32_t kp, int32_t act, void* stream);

/* LayerNorm(x (+ residual, may be NULL)) as mmr_layernorm_bf16 / mmr_add_layernorm_bf16, also
 * emitting the row as an MX-fp8 activation operand (q8 [rows][c] e4m3 + layout-0 scales,
 * rows % 256 == 0, c % 256 == 0), bit-identical to mmr_quantize_mxfp8 of y (the fp8 towers' QKV / FFN1
 * inputs). */
mmr_status mmr_layernorm_bf16_q8(const uint16_t* x, const uint16_t* residual, const float* gamma,
                                 const float* beta, uint16_t* y, uint8_t* q8, uint8_t* q8_scales, int64_t rows,
                                 int32_t c, float eps, void* stream);

/* mmr_layernorm_bf16_q8 with the operand's K padded to kp (kp % 256 == 0, kp >= c, c % 32 == 0; q8 is
 * [rows][kp], the padding written as zero bytes with zero scale bytes, bit-identical to
 * mmr_quantize_mxfp8(y, k=c, kp)), and y may be NULL when only the operand is consumed (the fp8 Swin
 * stages: C = 384 -> kp 512 for stage 3, C = 768 for stage 4). */
mmr_status mmr_layernorm_bf16_q8p(const uint16_t* x, const uint16_t* residual, const float* gamma,
                                  const float* beta, uint16_t* y, uint8_t* q8, uint8_t* q8_scales, int64_t rows,
                                  int32_t c, int32_t kp, float eps, void* stream);

/* Row LayerNorm over c channels (bf16 in/out, f32 math, gamma/beta f32). */
mmr_status mmr_layernorm_bf16(const uint16_t* x, const float* gamma, const float* beta,
                              uint16_t* y, int64_t rows, int32_t c, float eps, void* stream);

/* Post-LN residual block: y = LayerNorm(x + residual) (sum in f32), bf16 in / out.  BERT's
 * BertSelfOutput / BertOutput (HF modeling_bert; reference fusion.py:322-325 via AutoModel):
 * the attention-output and FFN2 GEMMs then need no residual epilogue. */
mmr_status mmr_add_layernorm_bf16(const uint16_t* x, const uint16_t* residual, const float* gamma,
                                  const float* beta, uint16_t* y, int64_t rows, int32_t c,
                                  float eps, void* stream);

/* y = LayerNorm(alpha * x + residual) with alpha a DEVICE f32 scalar (NULL = 1) and residual may be
 * NULL: PreFusionEnhancer's norm1(alpha * x + x2) (src/Model/fusion.py:34) on the vectorised
 * row kernel.  bf16 in / out, contiguous rows of c channels (c % 8 == 0). */
mmr_status mmr_scaled_add_layernorm_bf16(const uint16_t* x, const float* alpha, const uint16_t* residual,
                                         const float* gamma, const float* beta, uint16_t* y, int64_t rows,
                                         int32_t c, float eps, void* stream);

/* mmr_scaled_add_layernorm_bf16 that also writes y as the next GEMM's MX-fp8 activation operand
 * (q8 [rows][c] e4m3 + q8_scales in the layout-0 image, bit-identical to mmr_quantize_mxfp8 of y):
 * the fusion stack's enhanced tokens feeding the folded cross projections (config 5, fp8 towers).
 * rows % 256 == 0, c % 256 == 0. */
mmr_status mmr_scaled_add_layernorm_bf16_q8(const uint16_t* x, const float* alpha, const uint16_t* residual,
                                            const float* gamma, const float* beta, uint16_t* y, uint8_t* q8,
                                            uint8_t* q8_scales, int64_t rows, int32_t c, float eps, void* stream);

/* BERT embeddings (HF BertEmbeddings): LN(word[id] + pos[l] + type[0]) -> bf16 (b*l, c). */
mmr_status mmr_bert_embed(const int64_t* ids, const float* word, const float* pos,
                          const float* type0, const float* gamma, const float* beta, uint16_t* y,
                          int32_t b, int32_t l, int32_t c, float eps, void* stream);
/* mmr_bert_embed also writing y as the first QKV GEMM's MX-fp8 activation operand (q8 [b*l][c] e4m3 +
 * layout-0 scales), bit-identical to mmr_quantize_mxfp8 of y (the fp8 BERT tower; c % 256 == 0,
 * c <= 1024, b*l % 256 == 0).  q8 / q8_scales NULL = mmr_bert_embed. */
mmr_status mmr_bert_embed_q8(const int64_t* ids, const float* word, const float* pos, const float* type0,
                             const float* gamma, const float* beta, uint16_t* y, uint8_t* q8, uint8_t* q8_scales,
                             int32_t b, int32_t l, int32_t c, float eps, void* stream);

/* BERT self-attention core (HF BertSelfAttention, eval): qkv bf16 (b*l, 3*h*dh) [q|k|v],
 * additive mask from mask01 (b, l) int64 (0 -> masked), softmax(q k^T / sqrt(dh)) v -> ctx bf16
 * (b*l, h*dh).  Any l; dh % 8 == 0, dh <= 192 (the mmr_mha kernel with a key mask).
 * A sequence whose mask01 row is all zero follows HF: finfo.min is added to every score, the softmax
 * is uniform, and every context row of that sequence is the mean of V over its l keys (finite, never
 * NaN; mmr_x3_attention does the same).  Sequences with at least one live key are unaffected. */
mmr_status mmr_bert_attention(const uint16_t* qkv, const int64_t* mask01, uint16_t* ctx,
                              int32_t b, int32_t l, int32_t h, int32_t dh, void* stream);

/* mmr_bert_attention that writes the context as the O-proj GEMM's MX-fp8 activation operand (q8
 * (b*l, h*dh) e4m3 + q8_scales in the layout-0 image, bit-identical to mmr_quantize_mxfp8 of ctx);
 * ctx may be NULL (no bf16 copy).  Config 5's fp8 BERT: no quantise pass between attention and
 * O-proj.  dh % 32 == 0, (b*l) % 256 == 0, (h*dh) % 256 == 0. */
mmr_status mmr_bert_attention_q8(const uint16_t* qkv, const int64_t* mask01, uint16_t* ctx, uint8_t* q8,
                                 uint8_t* q8_scales, int32_t b, int32_t l, int32_t h, int32_t dh, void* stream);

/* Swin (shifted-)window attention core (timm WindowAttention + cyclic shift, eval):
 * qkv bf16 (b*hw*hw, 3*c) in natural token order; the kernel applies roll(-shift), window
 * partition, q*dh^-0.5, k^T, + the dense bias from mmr_swin_attn_bias, softmax, v, window reverse
 * and roll(+shift) -> out bf16 (b*hw*hw, c).  ws*ws <= 64, head_dim 32. */
mmr_status mmr_swin_window_attention(const uint16_t* qkv, const float* bias, uint16_t* out,
                                     int32_t b, int32_t hw, int32_t c, int32_t heads, int32_t ws,
                                     int32_t shift, void* stream);
/* mmr_swin_window_attention writing its output as the proj GEMM's MX-fp8 activation operand (q8
 * [b*hw*hw][kp] e4m3 + layout-0 scales, K padded to kp with zero bytes / zero scale bytes) instead of
 * bf16 rows, bit-identical to mmr_quantize_mxfp8 of the bf16 output (the fp8 Swin stages 3-4; rows %
 * 256 == 0, kp % 256 == 0, kp >= c). */
mmr_status mmr_swin_window_attention_q8(const uint16_t* qkv, const float* bias, uint8_t* q8, uint8_t* q8_scales,
                                        int32_t b, int32_t hw, int32_t c, int32_t kp, int32_t heads, int32_t ws,
                                        int32_t shift, void* stream);
/* Dense additive attention bias for one Swin block, built once at load: f32
 * [t][heads][64][64], t = 4 window types when shift > 0 (2*last-row + last-col), else 1:
 * relative_position_bias_table[(yi-yj+ws-1)*(2ws-1) + (xi-xj+ws-1)][head] (timm index), + -100
 * where the shift regions of i and j differ, -FLT_MAX for padded keys j >= ws*ws. */
mmr_status mmr_swin_attn_bias(const float* relpos_table, float* bias, int32_t heads, int32_t ws,
                              int32_t hw, int32_t shift, void* stream);

/* Fused Swin MLP sub-block for C in {96, 192} (the memory-bound stages 1-2):
 * y = x + fc2(GELU(fc1(LayerNorm(x)))) with the 4C hidden activation kept on chip.
 * x, y bf16 (tokens, C) (x != y); ln_g/ln_b, b1 (4C), b2 (C) f32; `pack` = weights repacked once by
 * mmr_swin_mlp_pack from fc1.weight [4C][C] and fc2.weight [C][4C] (bf16) into
 * mmr_swin_mlp_pack_elems(C) bf16 elements. */
int64_t mmr_swin_mlp_pack_elems(int32_t c);
mmr_status mmr_swin_mlp_pack(const uint16_t* w1, const uint16_t* w2, uint16_t* pack, int32_t c,
                             void* stream);
mmr_status mmr_swin_mlp(const uint16_t* x, const float* ln_g, const float* ln_b,
                        const uint16_t* pack, const float* b1, const float* b2, uint16_t* y,
                        int64_t tokens, int32_t c, float eps, void* stream);

/* Fused Swin attention sub-block for C = 96 (3 heads of 32, window 7; Swin-T stage 1):
 * y = x + proj(W-MSA(LayerNorm1(x))) with torch.roll shift, window partition / reverse,
 * relative-position bias and shift mask (timm SwinTransformerBlock, fusion.py:198-199).
 * x, y bf16 (b, hw, hw, 96) (x != y); `bias` = the block's dense table from mmr_swin_attn_bias;
 * `pack` = mmr_swin_attn_block_pack_bytes(96) bytes built once from attn.qkv.weight [288][96] /
 * .bias, attn.proj.weight [96][96] / .bias (bf16 weights, f32 vectors) and norm1.weight / .bias. */
int64_t mmr_swin_attn_block_pack_bytes(int32_t c);
mmr_status mmr_swin_attn_block_pack(const uint16_t* qkv_w, const float* qkv_b, const uint16_t* proj_w,
                                    const float* proj_b, const float* ln_g, const float* ln_b,
                                    void* pack, int32_t c, void* stream);
mmr_status mmr_swin_attn_block(const uint16_t* x, const void* pack, const float* bias, uint16_t* y,
                               int32_t b, int32_t hw, int32_t c, int32_t ws, int32_t shift, float eps,
                               void* stream);

/* Swin patch embedding im2col: image f32 NCHW (b,3,224,224) -> bf16 (b*56*56, 48) columns in
 * conv-weight order (cin, kh, kw) for a 4x4/s4 conv as a GEMM. */
mmr_status mmr_patch_im2col(const float* image, uint16_t* cols, int32_t b, int32_t cin,
                            int32_t hw, int32_t patch, void* stream);

/* Swin PatchMerging gather + LayerNorm(4c): x bf16 (b, hw, hw, c) -> y bf16 (b*(hw/2)^2, 4c) in
 * timm order [x(0,0), x(1,0), x(0,1), x(1,1)]. */
mmr_status mmr_patch_merge_ln(const uint16_t* x, const float* gamma, const float* beta,
                              uint16_t* y, int32_t b, int32_t hw, int32_t c, float eps,
                              void* stream);
/* mmr_patch_merge_ln also (y may be NULL: instead) writing the merged row as the reduction GEMM's
 * MX-fp8 activation operand (q8 [rows][4c] e4m3 + layout-0 scales), bit-identical to
 * mmr_quantize_mxfp8 of y (the fp8 Swin stages 3-4: 4c = 768 / 1536; rows % 256 == 0, 4c % 256 == 0). */
mmr_status mmr_patch_merge_ln_q8(const uint16_t* x, const float* gamma, const float* beta, uint16_t* y,
                                 uint8_t* q8, uint8_t* q8_scales, int32_t b, int32_t hw, int32_t c, float eps,
                                 void* stream);

/* Swin head (fusion.py:263-265 with swin_norm = swin.norm): x bf16 (b, t, c) = backbone tokens
 * BEFORE the final norm.  patches = LN(LN(x)) f32 (b,t,c), global = mean_t LN(x) f32 (b,c),
 * pool = mean over the t+1 rows [global; patches] f32 (b,c) — the image head's pooled input
 * (model.py:463-468: mean(cat[proj(g), proj(p)]) == proj(mean(cat[g, p])) for an affine proj).
 * Any output may be NULL. */
mmr_status mmr_swin_head(const uint16_t* x, const float* gamma, const float* beta, float* patches,
                         float* global, float* pool, int32_t b, int32_t t, int32_t c, float eps,
                         void* stream);

/* Unmasked mean over l tokens (model.py:370, PAD included): x bf16 (b,l,c) -> f32 (b,c). */
mmr_status mmr_mean_tokens(const uint16_t* x, float* y, int32_t b, int32_t l, int32_t c,
                           void* stream);

/* Fused projection head: y = W2 . GELU(W1 . (Wp . x + bp) + b1) + b2 (model.py:365-373 proj then
 * MultiHeadMLP model.py:61-75), f32 weights/activations, optional L2 normalise of the result.
 * w2/b2/w1/b1 may be NULL (projection only).  x (b, cin) f32, y (b, d) f32. */
mmr_status mmr_proj_head(const float* x, const float* wp, const float* bp, const float* w1,
                         const float* b1, const float* w2, const float* b2, float* y, int32_t b,
                         int32_t cin, int32_t d, int32_t l2norm, void* stream);

/* Small exact-f32 linear on strided rows: y[i*ldy + o] = act(x[i*ldx + :] . w[o][:] + bias[o])
 * (+ residual[i*ldr + o]); residual may alias y (in-place x += f(x)).  cin % 16 == 0,
 * cout % 32 == 0, ldx % 4 == 0.  The per-query vectors of the fusion stack (model.py:431-449). */
mmr_status mmr_linear_f32(const float* x, int64_t ldx, const float* w, const float* bias,
                          const float* residual, int64_t ldr, float* y, int64_t ldy, int32_t b,
                          int32_t cin, int32_t cout, int32_t act, void* stream);

/* nbatch independent mmr_linear_f32 problems in one launch; problem i reads x + i*bsx, w + i*bsw,
 * bias + i*bsb, residual + i*bsr and writes y + i*bsy (element strides; bsx, bsw % 4 == 0): the
 * per-query work of all fusion layers at once (each layer has its own weights). */
mmr_status mmr_linear_f32_batched(const float* x, int64_t ldx, int64_t bsx, const float* w, int64_t bsw,
                                  const float* bias, int64_t bsb, const float* residual, int64_t ldr,
                                  int64_t bsr, float* y, int64_t ldy, int64_t bsy, int32_t nbatch, int32_t b,
                                  int32_t cin, int32_t cout, int32_t act, void* stream);

/* ---------------------------------------------------------------- multimodal fusion stack */
/* model_type="multimodal": CrossModalFusion (src/Model/fusion.py:334-471) x num_fusion_layers +
 * the combiner (src/Model/model.py:375-459), eval.  Orchestrated host-side over these ops and
 * mmr_linear_bf16 / mmr_linear_f32. */

/* nn.MultiheadAttention core (no masks): per (batch, head) softmax(q k^T * scale) v.
 * q row (bi*lq + i) at q + row*ldq + head*dh (k, v likewise with lk); out (b*lq, ldo) bf16 and/or
 * mean_out (b, heads*dh) f32 = the mean over the lq query rows (either may be NULL, not both).
 * dh % 8 == 0, dh <= 192; strides multiples of 8 elements; any lq / lk (keys stream through LDS).
 * mean_out is bitwise deterministic for lq <= 128; longer query sets add per-128-row partials with
 * float atomics. */
mmr_status mmr_mha(const uint16_t* q, int64_t ldq, const uint16_t* k, int64_t ldk, const uint16_t* v,
                   int64_t ldv, uint16_t* out, int64_t ldo, float* mean_out, int32_t b, int32_t lq,
                   int32_t lk, int32_t heads, int32_t dh, float scale, void* stream);
/* mmr_mha emitting its output (also) as the next GEMM's MX-fp8 activation operand: e4m3 q8
 * [b*lq][heads*dh] + E8M0 scales in the layout-0 image of mmr_quantize_mxfp8 (bit-identical to
 * quantising the bf16 rows); out may be NULL.  head_dim % 32 == 0, b*lq % 256 == 0, heads*dh % 256 == 0. */
mmr_status mmr_mha_q8(const uint16_t* q, int64_t ldq, const uint16_t* k, int64_t ldk, const uint16_t* v, int64_t ldv,
                      uint16_t* out, int64_t ldo, float* mean_out, uint8_t* q8, uint8_t* q8_scales, int32_t b,
                      int32_t lq, int32_t lk, int32_t heads, int32_t dh, float scale, void* stream);
/* The attention weights nn.MultiheadAttention returns beside its output with its defaults (need_weights,
 * average_attn_weights; eval, no masks): probs[bi*lq + i][c] = (1 / heads) sum_h softmax_c(q_h[i] . k_h[c] * scale),
 * f32 — the reference's return_attention maps (src/Model/fusion.py:427,433, model.py:399).  q / k rows as
 * mmr_mha (bf16; one bf16 MFMA product per q.k, exact in f32), softmax and head average in f32; output row
 * (bi*lq + i) at probs + row*ldp, columns [0, lk) written, columns lk..ldp untouched (ldp >= lk, any
 * alignment of the rows).  dh % 8 == 0, dh <= 192; q / k strides multiples of 8 elements; any lq / lk >= 1
 * (keys stream from global memory: no bound on lk); heads <= 223 (per-head softmax statistics live in LDS;
 * MMR_ERR_UNSUPPORTED beyond).  No atomics, fixed head order: bitwise deterministic.  b == 0: no launch. */
mmr_status mmr_mha_probs(const uint16_t* q, int64_t ldq, const uint16_t* k, int64_t ldk, float* probs, int64_t ldp,
                         int32_t b, int32_t lq, int32_t lk, int32_t heads, int32_t dh, float scale, void* stream);

/* y = x + pos[row % l] -> bf16 (rows, c); x f32 (x_is_f32) or bf16; pos f32 [>= l][c]
 * (PreFusionEnhancer.pos_embed fusion.py:32). c % 8 == 0. */
mmr_status mmr_add_pos_bf16(const void* x, int32_t x_is_f32, const float* pos, uint16_t* y, int64_t rows,
                            int32_t l, int32_t c, void* stream);

/* mmr_add_pos_bf16 that also writes y as the next GEMM's MX-fp8 activation operand (as
 * mmr_scaled_add_layernorm_bf16_q8): the enhancer input x + pos feeding its in_proj GEMM (config 5).
 * rows % 256 == 0, c % 256 == 0. */
mmr_status mmr_add_pos_bf16_q8(const void* x, int32_t x_is_f32, const float* pos, uint16_t* y, uint8_t* q8,
                               uint8_t* q8_scales, int64_t rows, int32_t l, int32_t c, void* stream);

/* y = LayerNorm(alpha*x + residual) (+ post_scale*post), per row of c <= 1024 channels.
 * alpha / post_scale are DEVICE f32 scalars (learned parameters) or NULL (= 1); residual / post
 * may be NULL.  io_bf16: x, residual, y bf16 (else f32); post is always f32.  Row r uses parameter
 * set g = (r / group_div) % groups — gamma/beta + g*c, alpha/post_scale + g — so one launch
 * normalises the rows of several layers (groups = layers; group_div = 1 for [..][layer][c] rows,
 * = rows per layer for [layer][..][c]). */
mmr_status mmr_ln_rows(const void* x, int64_t ldx, const float* alpha, const void* residual, int64_t ldr,
                       const float* gamma, const float* beta, const float* post, int64_t ldp,
                       const float* post_scale, void* y, int64_t ldy, int64_t rows, int32_t c, float eps,
                       int32_t io_bf16, int32_t groups, int64_t group_div, void* stream);

/* f32 y = LayerNorm(alpha * x + residual) (alpha: a DEVICE f32 scalar or NULL = 1; residual may be NULL,
 * y may be NULL) that also writes xs, the x3 split GEMM's X operand: [hi | lo] bf16 rows 2 kp wide
 * (kp = mmr_x3_p8_kpad(c), zero columns c..kp), the split mmr_x3_split_rows would make of y.
 * c % 4 == 0, c <= 1024; rows 16-B aligned. */
mmr_status mmr_ln_rows_split(const float* x, int64_t ldx, const float* alpha, const float* residual, int64_t ldr,
                             const float* gamma, const float* beta, float* y, int64_t ldy, uint16_t* xs, int64_t rows,
                             int32_t c, float eps, void* stream);

/* seq (b, np+2, c) bf16 = [x1; patches_fused; x2] + pe[0..np+2) (fusion.py:468 + model.py:397);
 * x1, x2 f32 (b, c), patches_fused bf16 (b*np, c), pe f32 [>= np+2][c]. */
mmr_status mmr_assemble_seq(const float* x1, const uint16_t* patches_fused, const float* x2, const float* pe,
                            uint16_t* seq, int32_t b, int32_t np, int32_t c, void* stream);

/* mmr_assemble_seq written only as the combiner QKV GEMM's MX-fp8 activation operand (layout 0, as
 * mmr_quantize_mxfp8 of the bf16 sequence, bit-identical); b*(np+2) and c multiples of 256.
 * Replaces: the same cat + pos_encoder (reference src/Model/model.py:396-397) on the fp8 path. */
mmr_status mmr_assemble_seq_q8(const float* x1, const uint16_t* patches_fused, const float* x2, const float* pe,
                               uint8_t* q8, uint8_t* q8_scales, int32_t b, int32_t np, int32_t c, void* stream);

/* y (b, c) f32 = x[i*ldx + 0..c) (bf16 rows, e.g. the CLS token of each sequence). */
mmr_status mmr_rows_to_f32(const uint16_t* x, int64_t ldx, float* y, int32_t b, int32_t c, void* stream);

/* ---------------------------------------------------------------- fp32-faithful tower mode ("x3") */
/* The towers and the multimodal head with f32 activations and every contraction on bf16 MFMA with
 * three-term splits (a = a_hi + a_lo, a.b ~= a_hi.b_hi + a_hi.b_lo + a_lo.b_hi in f32, ~2^-17
 * relative per product); LayerNorm / softmax (expf) / GELU (erff) / means in f32.  The reference runs
 * the same towers in fp32 (src/Model/fusion.py:198-199, 322-325; model.py:365-479): this mode holds the
 * end-to-end lists to BASELINE.md §3's bar.  All activations f32. */

/* y = act(x @ W^T + bias) (+ residual) for any m: x (m, k) rows at stride ldx, W given as its bf16
 * split w_hi = bf16(W), w_lo = bf16(W - w_hi) ([n][k] each, contiguous); act 0 none, 1 GELU(erf).
 * k % 32 == 0; residual may alias y. */
mmr_status mmr_x3_linear(const float* x, int64_t ldx, const uint16_t* w_hi, const uint16_t* w_lo, const float* bias,
                         const float* residual, int64_t ldr, float* y, int64_t ldy, int64_t m, int32_t n, int32_t k,
                         int32_t act, void* stream);
/* The same linear at the 8-phase GEMM's rate: the split operands X = [x_hi | x_lo] and W = [w_hi | w_lo]
 * (bf16 rows, each segment kp = mmr_x3_p8_kpad(k) wide: k rounded up to 128, zero padding; 0 = k not
 * taken) in ONE GEMM whose K-tiles hold 32 k of both segments and issue x_hi.w_hi + x_hi.w_lo + x_lo.w_hi
 * into f32 accumulators (each operand staged once).
 * mmr_x3_split_rows writes X ([m][2 kp] bf16, caller-allocated) from f32 x rows at stride ldx;
 * mmr_ln_rows_split, the attention _xs forms below and a split output (out_hilo) write the same rows.
 * mmr_x3_linear_p8 takes X and the weight image W ([npad][2 kp] bf16, built once at load, npad =
 * mmr_x3_p8_npad(n): n itself when it is a multiple of 192 or 256, else n rounded up to 192 with zero
 * rows; 0 = n not taken) and writes y (m, n) f32 contiguous: m % 256 == 0, act 0 / 1 (GELU, erf), bias
 * NULL or npad floats (zero-padded), residual (m, n) f32 contiguous or NULL (may be y).
 * out_hilo != 0: y is written as the NEXT x3 GEMM's X operand, [y_hi | y_lo] bf16 rows 2 n wide
 * (the split of the f32 value mmr_x3_split_rows would make, bit for bit); needs n % 384 == 0 and no
 * residual — a FFN1 -> FFN2 pair then skips the f32 round trip and the split pass. */
int32_t mmr_x3_p8_kpad(int32_t k);
int32_t mmr_x3_p8_npad(int32_t n);
mmr_status mmr_x3_split_rows(const float* x, int64_t ldx, int64_t m, int32_t k, uint16_t* xs, void* stream);
mmr_status mmr_x3_linear_p8(const uint16_t* xs, const uint16_t* w2, const float* bias, const float* residual, void* y,
                            int64_t m, int32_t n, int32_t k, int32_t act, int32_t out_hilo, void* stream);
/* Attention core (nn.MultiheadAttention / BERT self-attention, eval): per (batch, head)
 * softmax(q k^T * scale (+ key mask)) v; rows as mmr_mha (q row bi*lq + i at q + row*ldq + head*dh);
 * mask01 (b, lk) int64 or NULL (0 -> key excluded, HF's additive finfo.min); out (b*lq, ldo) and/or
 * mean_out (b, heads*dh) = mean over the lq query rows (deterministic).  dh % 8 == 0, dh <= 128. */
mmr_status mmr_x3_attention(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                            float* out, int64_t ldo, float* mean_out, const int64_t* mask01, int32_t b, int32_t lq,
                            int32_t lk, int32_t heads, int32_t dh, float scale, void* stream);
/* mmr_mha_probs on f32 rows (the x3 mode's attention maps): q and k split hi / lo in registers and each
 * q.k summed as hi.hi + hi.lo + lo.hi, exactly as mmr_x3_attention's scores; softmax (mmr::exp_acc) and head
 * average in f32.  dh % 8 == 0, dh <= 128; strides multiples of 4 elements. */
mmr_status mmr_x3_attention_probs(const float* q, int64_t ldq, const float* k, int64_t ldk, float* probs, int64_t ldp,
                                  int32_t b, int32_t lq, int32_t lk, int32_t heads, int32_t dh, float scale,
                                  void* stream);
/* Swin (shifted-)window attention as mmr_swin_window_attention on f32 qkv (b*hw*hw, 3c) -> out
 * (b*hw*hw, c), q scaled by dh^-0.5 before q k^T (timm), bias from mmr_swin_attn_bias.  head_dim <= 32. */
mmr_status mmr_x3_swin_window_attention(const float* qkv, const float* bias, float* out, int32_t b, int32_t hw,
                                        int32_t c, int32_t heads, int32_t ws, int32_t shift, void* stream);
/* The two above writing their output as the x3 split GEMM's X operand instead (the O-proj / proj
 * input): xs = [hi | lo] bf16 rows 2 kp wide, kp = mmr_x3_p8_kpad(heads*dh) (columns heads*dh..kp zero),
 * the split mmr_x3_split_rows would make of the f32 output. */
mmr_status mmr_x3_attention_xs(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                               uint16_t* xs, float* mean_out, const int64_t* mask01, int32_t b, int32_t lq, int32_t lk,
                               int32_t heads, int32_t dh, float scale, void* stream);  /* mean_out may be NULL */
mmr_status mmr_x3_swin_window_attention_xs(const float* qkv, const float* bias, uint16_t* xs, int32_t b, int32_t hw,
                                           int32_t c, int32_t heads, int32_t ws, int32_t shift, void* stream);
/* Patch-embed im2col, f32: (b, cin, hw, hw) -> (b*(hw/patch)^2, kp) columns (k = c*p^2 + ky*p + kx, zero
 * for k >= cin*p^2). */
mmr_status mmr_x3_patch_im2col(const float* image, float* cols, int32_t b, int32_t cin, int32_t hw, int32_t patch,
                               int32_t kp, void* stream);
/* PatchMerging gather (timm order) + LayerNorm(4c), f32 in / out; 4c <= 4096. */
mmr_status mmr_x3_patch_merge_ln(const float* x, const float* gamma, const float* beta, float* y, int32_t b,
                                 int32_t hw, int32_t c, float eps, void* stream);
/* The same writing the reduction linear's x3 split operand instead: xs = [hi | lo] bf16 rows 2 kp wide,
 * kp = mmr_x3_p8_kpad(4c) (zero columns 4c..kp); c % 4 == 0, 16-B aligned pointers. */
mmr_status mmr_x3_patch_merge_ln_xs(const float* x, const float* gamma, const float* beta, uint16_t* xs, int32_t b,
                                    int32_t hw, int32_t c, float eps, void* stream);
/* BERT embeddings LN((word[id] + type[0]) + pos[l]) -> f32 (b*l, c), c <= 1024. */
mmr_status mmr_x3_bert_embed(const int64_t* ids, const float* word, const float* pos, const float* type0,
                             const float* gamma, const float* beta, float* y, int32_t b, int32_t l, int32_t c, float eps,
                             void* stream);
/* y = x + pos[row % l], f32 (rows, c). */
mmr_status mmr_x3_add_pos(const float* x, const float* pos, float* y, int64_t rows, int32_t l, int32_t c, void* stream);
/* The same written as the x3 split GEMM's operand: xs = [hi | lo] bf16 rows 2 kp wide (kp =
 * mmr_x3_p8_kpad(c), zero columns c..kp), plus the f32 rows y when y != NULL; c % 4 == 0, 16-B aligned. */
mmr_status mmr_x3_add_pos_split(const float* x, const float* pos, float* y, uint16_t* xs, int64_t rows, int32_t l,
                                int32_t c, void* stream);
/* seq (b, np+2, c) f32 = [x1; patches_fused; x2] + pe. */
mmr_status mmr_x3_assemble_seq(const float* x1, const float* patches_fused, const float* x2, const float* pe,
                               float* seq, int32_t b, int32_t np, int32_t c, void* stream);
/* The same written only as the combiner QKV GEMM's x3 split operand rows (as mmr_x3_add_pos_split). */
mmr_status mmr_x3_assemble_seq_split(const float* x1, const float* patches_fused, const float* x2, const float* pe,
                                     uint16_t* xs, int32_t b, int32_t np, int32_t c, void* stream);
/* fp32-faithful fused Swin MLP (csrc/x3_mlp.hip): y = x + fc2(GELU_erf(fc1(LN(x)))) over tokens x (tokens, c)
 * f32 (c in {96, 192}; y != x, 16-B aligned), both linears on bf16x3 MFMA, the hidden never leaving the CU.
 * pack: mmr_x3_swin_mlp_pack_elems(c) bf16 elements, built once from the f32 fc1.weight [4c][c] and
 * fc2.weight [c][4c] by mmr_x3_swin_mlp_pack (0 elements / MMR_ERR_UNSUPPORTED for other c). */
int64_t mmr_x3_swin_mlp_pack_elems(int32_t c);
/* fp32-faithful row-linear for the narrow Swin stages (csrc/x3_mlp.hip): y (tokens, n) f32 = LN(x) W^T + b
 * (+ residual) with x f32 (tokens, c) and its LayerNorm (ln_g, ln_b), or = xs W^T + b (+ residual) with xs
 * the x3 split-operand rows [hi | lo] (tokens, 2 kp), kp = mmr_x3_p8_kpad(c) (the window attention's _xs
 * output) — exactly one of x / xs.  bf16x3 MFMA, W^T streamed through LDS.  c in {96, 192}, n % 32 == 0,
 * n <= 4096 (c = 96: n > 64); pack = mmr_x3_rowlin_pack_elems(n, c) bf16 elements built once from the f32
 * weight [n][c] by mmr_x3_rowlin_pack. */
int64_t mmr_x3_rowlin_pack_elems(int32_t n, int32_t c);
mmr_status mmr_x3_rowlin_pack(const float* w, uint16_t* pack, int32_t n, int32_t c, void* stream);
mmr_status mmr_x3_rowlin(const float* x, const uint16_t* xs, const float* ln_g, const float* ln_b, const uint16_t* pack,
                         const float* bias, const float* residual, float* y, int64_t tokens, int32_t n, int32_t c,
                         float eps, void* stream);
mmr_status mmr_x3_swin_mlp_pack(const float* w1, const float* w2, uint16_t* pack, int32_t c, void* stream);
/* fp32-faithful fused Swin attention sub-block for C = 96 (3 heads of 32, window 7; Swin-T stage 1,
 * csrc/x3_sab.hip): y = x + proj(W-MSA(LayerNorm1(x))) with torch.roll shift, window partition / reverse,
 * relative-position bias and shift mask (timm SwinTransformerBlock, fusion.py:198-199) in f32, every
 * contraction on bf16x3 MFMA — the x3_rowlin (norm1 + qkv) -> x3 window attention -> x3_rowlin (proj +
 * residual) chain in one pass.  x, y f32 (b, hw, hw, 96) (x != y, 16-B aligned); `bias` = the block's dense
 * table from mmr_swin_attn_bias; `pack` = mmr_x3_swin_attn_block_pack_bytes(96) bytes built once from the
 * f32 attn.qkv.weight [288][96] / .bias, attn.proj.weight [96][96] / .bias and norm1.weight / .bias
 * (0 bytes / MMR_ERR_UNSUPPORTED for other c). */
int64_t mmr_x3_swin_attn_block_pack_bytes(int32_t c);
mmr_status mmr_x3_swin_attn_block_pack(const float* qkv_w, const float* qkv_b, const float* proj_w, const float* proj_b,
                                       const float* ln_g, const float* ln_b, void* pack, int32_t c, void* stream);
mmr_status mmr_x3_swin_attn_block(const float* x, const void* pack, const float* bias, float* y, int32_t b, int32_t hw,
                                  int32_t c, int32_t ws, int32_t shift, float eps, void* stream);
mmr_status mmr_x3_swin_mlp(const float* x, const float* ln_g, const float* ln_b, const uint16_t* pack, const float* b1,
                           const float* b2, float* y, int64_t tokens, int32_t c, float eps, void* stream);
/* fp32-faithful Swin stem (csrc/x3_mlp.hip): y (b, hw/4, hw/4, 96) f32 = LayerNorm(Conv2d(3, 96, 4, stride 4)
 * (img) + bias) (timm PatchEmbed with its norm) for img (b, 3, hw, hw) f32 NCHW, the conv on bf16x3 MFMA, one
 * pass (no im2col rows).  hw % 4 == 0, (hw/4)^2 % 32 == 0, 16-B aligned pointers.  pack:
 * mmr_x3_patch_embed_pack_elems() bf16 elements built once from the f32 conv weight [96][3*4*4] by
 * mmr_x3_patch_embed_pack. */
int64_t mmr_x3_patch_embed_pack_elems(void);
mmr_status mmr_x3_patch_embed_pack(const float* w, uint16_t* pack, void* stream);
mmr_status mmr_x3_patch_embed_ln(const float* img, int32_t b, int32_t hw, const uint16_t* pack, const float* bias,
                                 const float* ln_g, const float* ln_b, float eps, float* y, void* stream);
/* The bf16 towers' stem on the same pack: y (b, hw/4, hw/4, 96) bf16 = LayerNorm(conv(img) + bias) with the
 * pixels rounded to bf16 and one bf16 product with the pack's hi image (= the bf16 conv weight), the
 * bias and LayerNorm on the f32 accumulators; replaces mmr_patch_im2col + the GEMM + mmr_layernorm_bf16
 * (timm PatchEmbed, fusion.py:198-199). */
mmr_status mmr_patch_embed_ln_bf16(const float* img, int32_t b, int32_t hw, const uint16_t* pack, const float* bias,
                                   const float* ln_g, const float* ln_b, float eps, uint16_t* y, void* stream);
/* y (b, c) = (extra[b] + sum_t x[b][t]) / (l + 1) with extra (b, c), or sum_t x[b][t] / l when extra is
 * NULL; x (b, l, c) f32, summed in token order (unmasked token mean, model.py:370; the Swin global /
 * pooled means, fusion.py:263-265, model.py:463-468). */
mmr_status mmr_x3_mean_rows(const float* x, const float* extra, float* y, int32_t b, int32_t l, int32_t c,
                            void* stream);
/* y (b, c) = x[i*ldx + 0..c), f32 (the CLS rows, fusion.py:447). */
mmr_status mmr_x3_gather_rows(const float* x, int64_t ldx, float* y, int32_t b, int32_t c, void* stream);

/* ---------------------------------------------------------------- classifier head / predict() tail */
/* The reference's classification head on the joint embedding and the tail of its predict()
 * (src/Model/model.py:271-277, 481, 491-537), eval (the Dropouts are identities), csrc/cls_head.hip:
 *   logits (b, c) f32 = W2 GELU_erf(W1 x + b1) + b2,  W1 [h][d], W2 [c][h]
 *   probs  (b, c) f32 = 1 / (1 + exp(-logits))
 *   preds  (b, c) i32 = probs >= threshold
 *   topk_vals / topk_idx (b, k) f32 / i32: the k largest probs per row, ordered by (prob desc, class asc)
 * One precision whatever the tower mode: f32 activations, both contractions on bf16x3 MFMA (as
 * mmr_linear_x3), no atomics, and a row's logits do not depend on the rest of the batch (same bits for any
 * b).  d % 128 == 0, d <= 1024, h == 4 d runs one fused pass with the hidden kept on chip plus a finishing
 * pass; other geometries (d % 16 == 0, h % 32 == 0) run mmr_linear_x3 / mmr_linear_f32 twice and the same
 * finishing pass.  1 <= c <= 256 (beyond: MMR_ERR_UNSUPPORTED); x rows f32 at stride ldx (>= d, % 4 == 0),
 * 16-B aligned.
 * images: mmr_classifier_pack_bytes(d, h, c) bytes (0: geometry not built), built once from the f32
 *   weights by mmr_classifier_pack; the layout is private to the library.
 * work:   mmr_classifier_work_bytes(b, d, h, c) bytes of scratch, owned by the caller, 16-B aligned.
 * probs, preds, topk_vals, topk_idx may each be NULL (not computed / not written); with a top-K output
 * 1 <= k <= c.  All outputs are dense.  b == 0: no launch. */
int64_t mmr_classifier_pack_bytes(int32_t d, int32_t h, int32_t c);
mmr_status mmr_classifier_pack(const float* w1, const float* w2, void* images, int32_t d, int32_t h, int32_t c,
                               void* stream);
int64_t mmr_classifier_work_bytes(int32_t b, int32_t d, int32_t h, int32_t c);
mmr_status mmr_classifier_head(const float* x, int64_t ldx, const void* images, const float* b1, const float* b2,
                               void* work, float* logits, float* probs, int32_t* preds, float* topk_vals,
                               int32_t* topk_idx, int32_t b, int32_t d, int32_t h, int32_t c, int32_t k,
                               float threshold, void* stream);

/* ---------------------------------------------------------------- classifier evaluation */
/* The reference's evaluation of its classifier (src/Evaluate/eval_on_test.py; Trainner/train.py:621-681) on
 * device, csrc/cls_eval.hip: scores (n, c) f32 rows at stride lds (>= c; probabilities or logits, any finite
 * values; -0 == +0, denormals are distinct scores), label_bits (n) uint64 (bit j = the sample has class j).
 * Result rows 0 .. c - 1 are the classes, row c the n * c flattened (score, label) pairs (sklearn's
 * average='micro').  Per row, with the distinct scores in descending order as tie groups, tp / fp = positives /
 * negatives scoring >= a group's value, dtp / dfp = the group's own:
 *   counts (c + 1, 4) int64: n_pos P, n_neg Nn, A = sum over groups of dfp (2 (tp - dtp) + dtp) = 2 #(pos > neg) +
 *     #(pos == neg) (AUROC = A / (2 P Nn)), the number of distinct scores
 *   ap_sum (c + 1) f64 = sum over groups of dtp * (tp / (tp + fp)) (AP = ap_sum / P), summed in a fixed order
 *   best_thr (c + 1) f32, best_f1 (c + 1) f64: _find_best_thresholds — over the distinct scores the maximum of
 *     f1 = (2 p r) / ((p + r) + 1e-8), p = tp / (tp + fp), r = tp / P (1.0 when P == 0), every operation rounded
 *     on its own in f64; equal f1: the lowest score
 *   confusion (c + 1, 3) int64 = tp, fp, fn of `score > threshold` against `thresholds` (c) f32 when given, else
 *     against best_thr (row c: the sums over the classes)
 *   nonfinite (1) int64 = the number of NaN / infinite scores; the other outputs are meaningless when it is not 0
 * 1 <= c <= 64, n >= 1, n * c < 2^31.  work: mmr_cls_eval_work_bytes(n, c) bytes (0: shape not taken) of scratch
 * owned by the caller, 16-B aligned.  All pointers device, asynchronous on `stream`; integer results and
 * fixed-order f64 sums only: two runs give identical bytes. */
int64_t mmr_cls_eval_work_bytes(int64_t n, int32_t c);
mmr_status mmr_cls_eval(const float* scores, int64_t lds, const uint64_t* label_bits, int64_t n, int32_t c,
                        const float* thresholds, int64_t* counts, double* ap_sum, float* best_thr, double* best_f1,
                        int64_t* confusion, int64_t* nonfinite, void* work, void* stream);

/* ---------------------------------------------------------------- attention explanations */
/* The attention family of the reference's ExplanationEngine.explain (src/Model/explain.py:825-947) for every sample
 * of a batch, csrc/explain.hip.  Inputs, f32, rows at unit column stride, batch / row strides in elements:
 * txt2img (b, lt, np), img2txt (b, np, lt), comb (b, lc_rows, lc_cols) — each may be NULL (its outputs are then not
 * written); t = the text length (txt_feats.shape[1]).  Per sample, every mean an f64 sum in a fixed order rounded to
 * f32 once, the rest f32 without contraction:
 *   p_txt (b, np) = column mean of txt2img;  t_img (b, lt) = column mean of img2txt
 *   p_comb (b, np), lc >= np only: lc == np the column mean, else the window of np consecutive columns with the
 *     largest mass (f64 column sums, ties: the lowest offset) — all zeros when max / (total + 1e-12) < 0.06, else
 *     the chosen columns' means
 *   t_comb (b, ltc), ltc = min(t, lc): lc == t the column mean; lc > t the same search over row sums (windows of t
 *     rows, ratio 0.0) and the chosen rows' means; lc < t the row means min-max normalised to [0, 1] (the uniform
 *     1 / lc when |max - min| < 1e-8)
 *   final_patch (b, np) = minmax(0.6 p_txt + 0.4 p_comb), or of the one that exists; final_token (b, min(lt, ltc))
 *     the same from t_img and t_comb trimmed to the shorter (lengths lt / ltc when only one exists);
 *     minmax(x) = (x - min) / ((max - min) + 1e-8f)
 *   map_txt2img, map_comb, map_final (b, h, w), each may be NULL: compute_attention_map of p_txt, p_comb,
 *     final_patch — minmax, viewed G x G, bilinear to (h, w) as F.interpolate(align_corners=False)
 *   offsets (b, 2) int32 = the chosen column / row offsets (0 for a plain mean, -1 where no vector)
 *   comb_absmax (b, 2) = max |p_comb|, max |t_comb| (the caller drops comb_img at <= 1e-8 and refuses a t_comb
 *     that is all <= 1e-7: steps 3-5 of compute_comb_token_vector are not built)
 *   nonfinite (1) int64 = the number of NaN / infinite entries of p_txt, t_img, p_comb, t_comb
 * MMR_ERR_INVALID before any launch: np outside 1..1024, or not a perfect square with a heat map asked for; lt or lc
 * outside 1..4096; comb not square; h * w outside 1..65536 with a heat map; a heat map not 16-B aligned; a NULL
 * output for a map that is given.  work: mmr_explain_attention_work_bytes(b, lt, np, lc) bytes (0: shape not
 * taken), 16-B aligned, needed with comb.  No float atomics: two runs give identical bytes. */
int64_t mmr_explain_attention_work_bytes(int32_t b, int32_t lt, int32_t np, int32_t lc);
mmr_status mmr_explain_attention(const float* txt2img, int64_t t2i_bs, int64_t t2i_rs, const float* img2txt,
                                 int64_t i2t_bs, int64_t i2t_rs, const float* comb, int64_t comb_bs, int64_t comb_rs,
                                 int32_t b, int32_t lt, int32_t np, int32_t lc_rows, int32_t lc_cols, int32_t t,
                                 int32_t h, int32_t w, float* p_txt, float* t_img, float* p_comb, float* t_comb,
                                 float* final_patch, float* final_token, float* map_txt2img, float* map_comb,
                                 float* map_final, int32_t* offsets, float* comb_absmax, int64_t* nonfinite,
                                 void* work, void* stream);

/* ---------------------------------------------------------------- map alignment */
/* The reference's compare_maps (src/Helpers/helper.py:173-209) for p pairs (pa[i], pb[i]) (int64) over n maps of hw
 * f32 pixels at stride ld, csrc/map_align.hip.  -0 == +0; k[j] = max(1, int(hw * frac_j)) for nf <= 4 fractions.
 * Per map:
 *   ranks2 (n, hw) uint32 = 2 x the average rank (scipy rankdata) of every pixel
 *   thresholds (n, nf) f32 = the k[j]-th largest value;  constant (n) int32 = all pixels equal
 *   mean (n), ssd (n) f64 = the mean and the sum of (x - mean)^2, summed in a fixed order
 * Per pair:
 *   pearson (p) f64 = sum (a - mean_a)(b - mean_b) / sqrt(ssd_a ssd_b)
 *   rank_sums (p, 3) int64 = S_ab, S_aa, S_bb of the centred doubled ranks c = ranks2 - (hw + 1) (exact)
 *   spearman (p) f64 = S_ab / sqrt(S_aa S_bb) (exactly 1 for a self-pair); pearson = spearman = 0.0 when either
 *     map is constant
 *   inter_union (p, nf, 2) int64 = the counts of (a >= ta_j) & (b >= tb_j) and of (a >= ta_j) | (b >= tb_j)
 *   skipped (p) int32 = 1 where pa[i] or pb[i] is outside [0, n): that pair's outputs are zeros
 * nonfinite (1) int64 = the number of NaN / infinite pixels (the other outputs are meaningless when it is not 0).
 * MMR_ERR_INVALID before any launch: n outside 1..65536, hw outside 1..65536, n * hw >= 2^31, k[j] outside 1..hw.
 * work: mmr_map_alignment_work_bytes(n, hw) bytes (0: shape not taken), 16-B aligned.  Integer results, order
 * statistics and fixed-order f64 sums only: two runs give identical bytes. */
int64_t mmr_map_alignment_work_bytes(int64_t n, int32_t hw);
mmr_status mmr_map_alignment(const float* maps, int64_t ld, int64_t n, int32_t hw, const int64_t* pa,
                             const int64_t* pb, int64_t p, int32_t nf, int32_t k0, int32_t k1, int32_t k2, int32_t k3,
                             uint32_t* ranks2, float* thresholds, int32_t* constant, double* mean, double* ssd,
                             double* pearson, double* spearman, int64_t* rank_sums, int64_t* inter_union,
                             int32_t* skipped, int64_t* nonfinite, void* work, void* stream);

/* ---------------------------------------------------------------- gradient explanations */
/* The backward kernels of the Grad-CAM / Integrated-Gradients maps (explain.py:170-427), csrc/explain_grad.hip: f32
 * throughout, every sum in a fixed order, no floating-point atomics — a sequence's (row's, map's) result does not
 * depend on what else is in the launch.
 *
 * Attention core, rows as mmr_x3_attention (q row bi*lq + i at q + row*ldq + head*dh; one ld per operand).
 * mmr_attention_fwd_f32: out = softmax(scale q k^T) v with every contraction on the f32-input MFMA (exp by ocml
 * expf): the forward the gradient pass differentiates.  mmr_attention_bwd_f32: given d_out = dL/dout, per
 * (sequence, head) S = scale q k^T and P = softmax(S) are recomputed (no probabilities are saved), then
 *   dV = P^T dO;  dP = dO V^T;  dS = P o (dP - rowsum(dP o P));  dQ = scale dS K;  dK = scale dS^T Q.
 * dq / dk / dv may each be NULL: that output is not computed (all NULL: no launch).  Columns [heads*dh, ld) of the
 * output rows are not written.
 * Limits: 1 <= lq, lk <= 128; dh % 8 == 0, 8 <= dh <= 96 — anything else MMR_ERR_UNSUPPORTED (nothing is clamped);
 * q, k, v, d_out 16-B aligned with row strides that are multiples of 4 and >= heads*dh, output strides >= heads*dh,
 * no NULL input (MMR_ERR_INVALID).  b == 0: no launch. */
mmr_status mmr_attention_fwd_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                                 float* out, int64_t ldo, int32_t b, int32_t lq, int32_t lk, int32_t heads, int32_t dh,
                                 float scale, void* stream);
mmr_status mmr_attention_bwd_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                                 const float* d_out, int64_t ldo, float* dq, int64_t lddq, float* dk, int64_t lddk,
                                 float* dv, int64_t lddv, int32_t b, int32_t lq, int32_t lk, int32_t heads, int32_t dh,
                                 float scale, void* stream);
/* LayerNorm backward over strided rows: for y = LN(z) gamma + beta, given the saved pre-norm row z and dy,
 * dz = rstd (g^ - mean(g^) - z^ mean(g^ o z^)) with g^ = gamma o dy, z^ = (z - mean z) rstd, rstd = 1 / sqrt(var z +
 * eps) (two-pass variance).  1 <= c <= 1024.  One parameter set (no groups). */
mmr_status mmr_ln_bwd_rows(const float* z, int64_t ldz, const float* gamma, const float* dy, int64_t lddy, float* dz,
                           int64_t lddz, int64_t rows, int32_t c, float eps, void* stream);
/* GELU (the exact erf form, ocml erff) over strided rows of the pre-activation h: dx = dy (Phi(h) + h phi(h)) (dx
 * NULL: not computed; else dy is required) and / or y = h Phi(h) (y NULL: not computed). */
mmr_status mmr_gelu_bwd_rows(const float* h, int64_t ldh, const float* dy, int64_t lddy, float* dx, int64_t lddx,
                             float* y, int64_t ldy, int64_t rows, int32_t c, void* stream);
/* Attribution vectors and maps.  grad (maps*steps, np, ci) contiguous: the rows of map m are m*steps + s; x (.., np,
 * ci) contiguous: map m reads x[(m / x_div) % x_mod] (maps ordered (sample, target): x_div = targets, x_mod = samples;
 * ordered (target, sample): x_div = 1, x_mod = samples); step_w (steps) the quadrature weights, NULL = 1.
 * t_e = (sum_s step_w[s] grad[m*steps + s, j, e]) x[.., j, e], steps summed in order; the step and channel sums
 * run in f64 in a fixed order and are rounded to f32 once.
 *   mode 0, Grad-CAM (explain.py:274-300): raw[m, j] = sum_e t_e (BEFORE the relu); map = relu, G x G, bilinear
 *     (align_corners=False) to (h, w), THEN (v - min) / ((max - min) + 1e-8f) over the pixels, then nan_to_num(0, 1, 0)
 *   mode 1, Integrated Gradients (:403-427): raw[m, j] = sum_e |t_e|; map = (a - min) / ((max - min) + 1e-8f) over
 *     the patches, clamp to [0, 1], nan_to_num(0, 1, 0), THEN bilinear to (h, w)
 * raw (maps, np) is always written; out_maps (maps, h, w) may be NULL (then np need not be a square).
 * MMR_ERR_INVALID: np outside 1..1024 or not a perfect square with out_maps; h*w outside 1..65536; steps outside
 * 1..1024. */
mmr_status mmr_attribution_maps(const float* grad, const float* x, const float* step_w, int64_t maps, int32_t steps,
                                int32_t x_div, int32_t x_mod, int32_t np, int32_t ci, int32_t mode, int32_t h, int32_t w,
                                float* raw, float* out_maps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MMR_H */
