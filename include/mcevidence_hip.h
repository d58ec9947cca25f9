/* mcevidence_hip.h -- C ABI of libmcevidence_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the k-nearest-neighbour evidence hot path of
 * yabebalFantaye/MCEvidence.  The reference has no FFI of its own: the seam is
 * the Python call into scikit-learn plus ~25 lines of NumPy
 * (reference MCEvidence.py:1093-1131).  Each entry point below names the
 * reference lines it replaces.  The Python binding a maintainer would add is
 * shown in INTEGRATION.md (ctypes; mcevidence_amd/_capi.py is that binding).
 *
 * Conventions
 *   - plain C types only; every matrix is C-contiguous (row-major) fp64.
 *   - *_f64      : pointers are HOST pointers to caller-owned buffers; the
 *                  library owns every device allocation it makes and frees it
 *                  before returning; nothing is retained after return.
 *   - *_f64_dev  : pointers are DEVICE pointers on the current HIP device
 *                  (e.g. torch tensors' data_ptr()); work is enqueued on
 *                  `stream` (a hipStream_t passed as void*, NULL = default
 *                  stream) and NOT synchronised; `ws` is caller-provided
 *                  scratch of at least mce_*_workspace_bytes().
 *   - return 0 on success, a negative MCE_ERR_* otherwise; mce_last_error()
 *     returns a thread-local message for the last failure on this thread.
 *   - one caller thread per device; calls are re-entrant across devices.  Several threads may share a device; the
 *     search / prune / symmetric modes then travel WITH the call (mce_options), not through the process-wide setters.
 *
 * Neighbour semantics (all entry points): Euclidean distance, the K smallest
 * per query in ascending order, ties broken by smaller reference index --
 * what `NearestNeighbors(...).kneighbors()` returns at MCEvidence.py:1104.
 */
#ifndef MCEVIDENCE_HIP_H
#define MCEVIDENCE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCE_ABI_VERSION 3     /* 2: per-call options (mce_options, *_opt), mce_last_search_stats; mce_options.verify and mce_verify_* were
                               * added compatibly (the field lies in what was reserved[0] = 0).
                               * 3 (round 6): every signature of 2 unchanged; NEW entry points (mce_last_verify_rows,
                               * mce_evidence_feed_part_dev_f64, mce_evidence_feed_whiten_dev_f64) and one changed DEFAULT:
                               * mce_options.verify = -1 now means "256 rows behind the fp16 filter" (0 still means off) */

#define MCE_OK 0
#define MCE_ERR_INVALID (-1)   /* bad argument (NULL, d<1, K<1, ...)        -> ValueError  */
#define MCE_ERR_K_RANGE (-2)   /* K larger than usable reference rows / MCE_MAX_K -> ValueError */
#define MCE_ERR_HIP (-3)       /* HIP runtime failure                        -> RuntimeError */
#define MCE_ERR_NO_DEVICE (-4) /* no gfx950 device visible                   -> RuntimeError */
#define MCE_ERR_WORKSPACE (-5) /* caller workspace too small                 -> ValueError  */
#define MCE_ERR_DIM_RANGE (-6) /* d larger than MCE_MAX_DIM                  -> ValueError  */
#define MCE_ERR_VERIFY (-7)    /* the re-check of sampled rows disagrees with the search (mce_options.verify) -> RuntimeError */

#define MCE_MAX_K 32    /* neighbours per query handled by the MFMA kernels (fp16 filter: 17..32 in two sweeps) */
#define MCE_MAX_DIM 63  /* dimensions handled by the one-to-four k-step fp16 filter (64..127: the deep fp16 filter, K <= 32 -- search mode 1: the
                           fp64 sweep; 128..1024: the fp64 sweep with the k dimension in blocks; feeders: d <= 127) */
#define MCE_GENERIC_MAX_K 1024   /* beyond MCE_MAX_K a plain exact kernel takes over, up to this many neighbours; rows up to */
#define MCE_GENERIC_MAX_DIM 1024 /* this long; larger -> MCE_ERR_K_RANGE / MCE_ERR_DIM_RANGE                                 */

/* self_mode: how the query set relates to the reference set.
 *   MCE_SELF_NONE    Y is a different set (cross evidence, MCEvidence.py:1093-1096, k0=0)
 *   MCE_SELF_INCLUDE Y row (self_offset+q) IS query q; it is reported with distance
 *                    exactly 0 in column 0 (what the auto path sees, MCEvidence.py:1099-1104)
 *   MCE_SELF_EXCLUDE same relation, but that row is skipped: the K columns are true
 *                    neighbours (equivalent to dropping column 0, `k0=1`, :1099)
 * self_offset is the reference row of query 0; query shards of one chain pass
 * their first global row (multi-GPU query sharding). */
#define MCE_SELF_NONE 0
#define MCE_SELF_INCLUDE 1
#define MCE_SELF_EXCLUDE 2

int mce_abi_version(void);
int mce_device_count(void);
const char *mce_last_error(void);

/* ---- host-pointer entry points (the literal drop-in) ------------------- */

/* Replaces NearestNeighbors(n_neighbors=K,...).fit(Y).kneighbors(X)
 * (MCEvidence.py:1093-1104).  dist[nq*K] ascending per row; idx[nq*K] int64 or NULL. */
int mce_knn_f64(const double *X, int64_t nq, const double *Y, int64_t nr, int32_t d, int32_t K,
                int32_t self_mode, int64_t self_offset, double *dist, int64_t *idx, int32_t device);

/* Replaces the volume loop + np.dot (MCEvidence.py:1107-1117):
 * dotp[k] = sum_j pi^(d/2) dist[j*ld+k]^d / Gamma(1+d/2) / w[j] * exp(fs[j]),  k in [k0,kmax).
 * Entries dotp[0..k0) are set to 0. */
int mce_dotp_f64(const double *dist, int64_t nq, int32_t ld, int32_t k0, int32_t kmax, int32_t d,
                 const double *w, const double *fs, double *dotp, int32_t device);

/* Fused path: search + reduction without returning the distances
 * (MCEvidence.py:1093-1117 in one call).  k0 = 1 -> auto evidence (Y must be the
 * set X was cut from; self excluded by index), k0 = 0 -> cross evidence.
 * dotp[kmax] as above.  dist_out (optional, may be NULL) receives the
 * [nq, kmax-k0] neighbour distances that entered the sum (columns k0..kmax-1 of
 * the reference's DkNN).  With ndev > 1 (devices[i] = HIP ordinal; NULL/0 -> device 0 only) the work is split over the
 * devices -- auto evidence of one set: the library's partition (mce_knn_dotp_part_f64), otherwise equal ranges of the
 * query rows -- by one host thread per device, and the partial sums are added ON THE HOST in device order (bitwise
 * reproducible run to run FOR A GIVEN DEVICE COUNT: the partition, hence the order of the sum, changes with the count;
 * SURVEY.md 8e's "alternatively").  The library itself has no RCCL dependency:
 * the one collective of a multi-PROCESS run -- an all-reduce of kmax doubles -- is the caller's
 * (mcevidence_amd/parallel.py: torch.distributed over RCCL), on the partial sums mce_knn_dotp_part_f64 returns. */
int mce_knn_dotp_f64(const double *X, int64_t nq, const double *Y, int64_t nr, int32_t d, int32_t kmax,
                     int32_t k0, int64_t self_offset, const double *w, const double *fs, double *dotp,
                     double *dist_out, const int32_t *devices, int32_t ndev);

/* Whole evidence() inner block with the feeders on the device too: replaces
 * get_covariance (MCEvidence.py:851-882), diagonalise_chain (:842-849) AND :1093-1117 in one call,
 * with ONE upload of the parameter columns.
 *   S1[n1, ld1] / S2[n2, ld2]: raw (un-whitened) parameter rows, row stride ld >= d, first d
 *       columns used.  S2 = NULL -> auto evidence (k0 = 1); otherwise cross evidence (k0 = 0).
 *   cov_mode 0 ("all"): covariance of the rows of S1 and S2 together; 1 ("single"): S1 whitened with
 *       its own eigen-system, S2 with ITS own (the reference's behaviour, :1080-1086).
 *       (Eigen-systems are canonical: eigenvalues descending, each eigenvector's largest component
 *       positive.  With cov_mode 1 AND S2 the result depends on that convention -- as the reference's
 *       depends on LAPACK's -- so the Python class keeps np.linalg.eig for that one combination.)
 *   Outputs: dotp[kmax]; *jacobian = sqrt(det cov) (of S1's covariance in mode 1);
 *       eigenvalues[d] (may be NULL), descending.  A non-positive eigenvalue -> MCE_ERR_INVALID (the reference
 *       raises ValueError: math domain error). */
int mce_evidence_feed_f64(const double *S1, int64_t n1, int64_t ld1, const double *S2, int64_t n2, int64_t ld2,
                          int32_t d, int32_t cov_mode, int32_t kmax, const double *w, const double *fs,
                          double *dotp, double *jacobian, double *eigenvalues, int32_t device);

/* One rank's share of mce_evidence_feed_f64 (multi-GPU, one process per GPU: SURVEY.md 8e; reference
 * MCEvidence.py:1034-1131): every rank passes the SAME arrays; this rank uploads them once, computes covariance, eigen-system
 * and whitening on its device like the single-rank call (identical on every rank), and searches only its share -- auto
 * evidence: the library's partition (mce_knn_dotp_part_f64); cross evidence: the rows [n1 part / nparts, n1 (part + 1) /
 * nparts) of S1 against all of S2.  dotp_part[kmax] = this rank's partial sums: ONE all-reduce(sum) over the ranks -- the
 * caller's (parallel.py: RCCL) -- completes them; jacobian / eigenvalues as in mce_evidence_feed_f64.
 * *checksum (may be NULL): a 64-bit fingerprint of the uploaded rows, weights and fs computed ON THE DEVICE (one extra
 * pass at HBM speed) -- ranks that were handed different samples are detected by comparing it, without hashing on the host. */
int mce_evidence_feed_part_f64(const double *S1, int64_t n1, int64_t ld1, const double *S2, int64_t n2, int64_t ld2,
                               int32_t d, int32_t cov_mode, int32_t kmax, const double *w, const double *fs,
                               int32_t part, int32_t nparts, double *dotp_part, double *jacobian, double *eigenvalues,
                               uint64_t *checksum, int32_t device);
/* Distributed k-d preparation of the pruned walk (round 6; reference: the `fit` of MCEvidence.py:1100-1101, which every rank of a
 * multi-GPU run repeated in full).  Rank `part` of nparts = 2, 4, 8, ... calls mce_prune_part_prepare_dev on the workspace it will
 * search with: the sorts that settle the tree's top log2(nparts) levels run over all rows, everything below them over the rank's
 * own subtree only.  On return *perm_count int32 values at ws + *perm_offset hold the final k-d order inside the rank's range
 * [*seg_lo, *seg_hi) (positions; the ranks' ranges follow each other in rank order and tile the array) and ZEROS elsewhere: an
 * all_gather of the ranges -- or one all-reduce(SUM) of the whole array -- over the ranks (the host's: torch.distributed over RCCL)
 * gives every rank the whole permutation -- bit for bit the single-GPU one -- and mce_knn_dotp_part_prepared_f64_dev then runs the rank's share of the
 * search like mce_knn_dotp_part_f64_dev, minus the sorts.  *perm_count = 0: nothing to exchange (the shape does not take the
 * pruned walk, nparts is not a power of two, the tree is too shallow) -- call mce_knn_dotp_part_f64_dev as before. */
int mce_prune_part_prepare_dev(const double *dY, int64_t nr, int32_t d, int32_t kmax, int32_t part, int32_t nparts,
                               size_t *perm_offset, int64_t *perm_count, int64_t *seg_lo, int64_t *seg_hi, void *ws,
                               size_t ws_bytes, void *stream);
/* 1: an auto-evidence search of this shape on nparts ranks takes the pruned walk AND its preparation can be distributed (plan only,
 * no device work): what a host asks before it chooses the three-step route */
int32_t mce_prune_part_applies(int64_t nr, int32_t d, int32_t kmax, int32_t nparts);
int mce_knn_dotp_part_prepared_f64_dev(const double *dY, int64_t nr, int32_t d, int32_t kmax, int32_t part, int32_t nparts,
                                       const double *d_w, const double *d_fs, double *d_dotp, void *ws, size_t ws_bytes,
                                       void *stream);

/* The same with the inputs ON THE DEVICE already (round 6; SURVEY.md 5: "one H2D + broadcast over xGMI instead of 8 PCIe
 * copies"): dS1 / dS2 / d_w / d_fs are device pointers on `device` (rows ld1 / ld2 doubles apart), produced on a stream the
 * caller has synchronised -- parallel.py uploads 1/W of the chain per rank and all_gathers it over RCCL.  Everything else
 * (host outputs included) as mce_evidence_feed_part_f64; the inputs are copied, not modified. */
int mce_evidence_feed_part_dev_f64(const double *dS1, int64_t n1, int64_t ld1, const double *dS2, int64_t n2, int64_t ld2,
                                   int32_t d, int32_t cov_mode, int32_t kmax, const double *d_w, const double *d_fs,
                                   int32_t part, int32_t nparts, double *dotp_part, double *jacobian, double *eigenvalues,
                                   uint64_t *checksum, int32_t device);
/* The feeders alone (auto evidence): upload, covariance of the n1 rows, Jacobi eigen-system, whitening -- and the whitened rows,
 * the weights and the likelihood terms left in DEVICE buffers of the caller's ([n1, d], [n1], [n1] doubles on `device`) instead of
 * being searched.  For hosts that run the search in several calls with collectives in between (the all-pairs-once partition:
 * parallel.py).  jacobian / eigenvalues / checksum as mce_evidence_feed_part_f64.  Reference: MCEvidence.py:1034-1060. */
int mce_evidence_feed_whiten_f64(const double *S1, int64_t n1, int64_t ld1, int32_t d, int32_t kmax, const double *w,
                                 const double *fs, double *d_X_out, double *d_w_out, double *d_fs_out, double *jacobian,
                                 double *eigenvalues, uint64_t *checksum, int32_t device);
/* ... with the inputs on the device already (as mce_evidence_feed_part_dev_f64) */
int mce_evidence_feed_whiten_dev_f64(const double *dS1, int64_t n1, int64_t ld1, int32_t d, int32_t kmax, const double *d_w,
                                     const double *d_fs, double *d_X_out, double *d_w_out, double *d_fs_out, double *jacobian,
                                     double *eigenvalues, uint64_t *checksum, int32_t device);

/* Many independent evidence problems in one call: the reference's Planck driver
 * runs MCEvidence(...).evidence() once per (data set, model, chain) -- ~600-2400 chains of 6k-100k
 * rows, D = 6-8 -- farmed over MPI ranks (planck_mcevidence.py:306-348).  One such chain fills a
 * fraction of the device, so here the problems of a batch are pipelined over several HIP streams
 * with two host synchronisations per batch.  Each problem has exactly the semantics of
 * mce_evidence_feed_f64 and yields bit-identical dotp / jacobian / eigenvalues.
 *   in : S1,n1,ld1,S2,n2,ld2,d,cov_mode,kmax,w,fs   (as mce_evidence_feed_f64; S2 = NULL -> auto)
 *   out: dotp[kmax], eigenvalues[d] (may be NULL), jacobian, status (MCE_OK or MCE_ERR_*)
 * Problems are spread over `devices` (NULL/0 -> device 0) balanced by n1*nr.  A failing problem does
 * not stop the others; the return value is the status of the first failing problem (its message in
 * mce_last_error(), prefixed "problem <i>: "), or MCE_OK. */
typedef struct mce_feed_problem {
    const double *S1; int64_t n1, ld1;
    const double *S2; int64_t n2, ld2;
    int32_t d, cov_mode, kmax, status;
    const double *w, *fs;
    double *dotp;
    double *eigenvalues;
    double jacobian;
} mce_feed_problem;

int mce_evidence_feed_batch_f64(mce_feed_problem *problems, int64_t nprob, const int32_t *devices, int32_t ndev);
size_t mce_feed_problem_size(void);   /* sizeof(mce_feed_problem) as built: lets a binding check its struct layout */
/* mce_evidence_feed_batch_f64 with S1, S2, w and fs of EVERY problem as device pointers on `device`, produced on a stream the caller
 * has synchronised (as for mce_evidence_feed_part_dev_f64; the inputs are copied, not modified).  dotp, eigenvalues, jacobian and
 * status stay host-side; streams, the wave limit, per-problem failures and the caller's mce_options (the run-time certificate
 * included) as in the host-pointer call. */
int mce_evidence_feed_batch_dev_f64(mce_feed_problem *problems, int64_t nprob, int32_t device);

/* Convergence batches (reference MCEvidence.py:1034-1131 with nbatch / brange: ln E from the FIRST S_b rows of the chain, for B
 * sizes) in one call, from one upload.  prefix[nprefix] (host array, non-decreasing, kmax + 1 <= prefix[b] <= n1) holds the sizes;
 * logl[n1] the log-likelihoods themselves, not yet shifted.  Entry b equals mce_evidence_feed_f64 on S1[:prefix[b]], S2,
 * w[:prefix[b]] and fs = logl[:p] - max(logl[:p]) -- except that with cov_mode 0 the eigen-system and the Jacobian are those of ALL
 * n1 (+ n2) rows and the same for every b, as in the reference (:1034-1037, :1057).  Cross evidence searches all of S2 for every
 * batch (:1075): one search serves them all.  cov_mode 1 with S2 -> MCE_ERR_INVALID (see mce_evidence_feed_f64).
 *   Outputs (host): dotp[nprefix * kmax], loglmax[b] = max(logl[:prefix[b]]) (NaN once a NaN lies below prefix[b], as np.amax),
 *       jacobian[nprefix].  A non-positive eigenvalue of any prefix -> MCE_ERR_INVALID, the prefix named in the message.
 *   mce_options.verify applies to each distinct search; mce_last_verify_rows() then counts the rows of all of them.
 * The host waits twice whatever nprefix is (for the covariances -- the eigen-solves are the host's -- and at the end); once with
 * mce_options.eig_mode = MCE_EIG_DEVICE (all the systems solved in one launch behind the covariances). */
#define MCE_MAX_PREFIX 256
int mce_evidence_feed_prefix_f64(const double *S1, int64_t n1, int64_t ld1, const double *S2, int64_t n2, int64_t ld2,
                                 int32_t d, int32_t cov_mode, int32_t kmax, const double *w, const double *logl,
                                 const int64_t *prefix, int32_t nprefix, double *dotp, double *loglmax, double *jacobian,
                                 int32_t device);
/* ... with S1 / S2 / w / logl as device pointers on `device`, produced on a stream the caller has synchronised (as for
 * mce_evidence_feed_part_dev_f64; the inputs are copied, not modified).  prefix and the outputs stay host-side. */
int mce_evidence_feed_prefix_dev_f64(const double *dS1, int64_t n1, int64_t ld1, const double *dS2, int64_t n2, int64_t ld2,
                                     int32_t d, int32_t cov_mode, int32_t kmax, const double *d_w, const double *d_logl,
                                     const int64_t *prefix, int32_t nprefix, double *dotp, double *loglmax, double *jacobian,
                                     int32_t device);

/* ---- device-pointer entry points (resident data, caller's stream) ------ */

size_t mce_knn_workspace_bytes(int64_t nq, int64_t nr, int32_t d, int32_t K);

int mce_knn_f64_dev(const double *dX, int64_t nq, const double *dY, int64_t nr, int32_t d, int32_t K,
                    int32_t self_mode, int64_t self_offset, double *d_dist, int64_t *d_idx, void *ws,
                    size_t ws_bytes, void *stream);

size_t mce_dotp_workspace_bytes(int64_t nq, int32_t kmax);

int mce_dotp_f64_dev(const double *d_dist, int64_t nq, int32_t ld, int32_t k0, int32_t kmax, int32_t d,
                     const double *d_w, const double *d_fs, double *d_dotp, void *ws, size_t ws_bytes,
                     void *stream);

/* Fused search + reduction on resident data; d_dotp[kmax] device, d_dist_out optional.
 * workspace: mce_knn_workspace_bytes(nq, nr, d, kmax-k0) + mce_dotp_workspace_bytes(nq, kmax). */
int mce_knn_dotp_f64_dev(const double *dX, int64_t nq, const double *dY, int64_t nr, int32_t d, int32_t kmax,
                         int32_t k0, int64_t self_offset, const double *d_w, const double *d_fs,
                         double *d_dotp, double *d_dist_out, void *ws, size_t ws_bytes, void *stream);

/* Multi-GPU building block for the auto evidence (queries = references, k0 = 1): the partial sums over
 * part `part` of `nparts` of the queries.  The LIBRARY chooses the partition -- contiguous rows for the
 * exhaustive sweep (the query shard of SURVEY.md section 8e; up to four parts of a set large enough for the symmetric sweep:
 * ranges of its sorted blocks, see mce_set_sym_mode), every nparts-th WAVE (64 queries: two k-d cells) of the pruned walk's
 * dispatch order, heaviest first (spatially compact work units, one shared ordering, statistically equal shares; a row-range
 * shard would go through the much less efficient separate-sets path; the heaviest waves of a part are served by several
 * workgroups each) -- the parts are disjoint and cover every row, so adding the
 * nparts results gives mce_knn_dotp_f64_dev's dotp up to summation order.  d_w / d_fs: all nr entries.
 * workspace: mce_knn_workspace_bytes(nr, nr, d, kmax-1) + mce_dotp_workspace_bytes(nr, kmax) -- the whole set's, whatever the
 * part (a row shard that would plan more reference splits than fit takes fewer). */
int mce_knn_dotp_part_f64_dev(const double *dY, int64_t nr, int32_t d, int32_t kmax, int32_t part, int32_t nparts,
                              const double *d_w, const double *d_fs, double *d_dotp, void *ws, size_t ws_bytes,
                              void *stream);
/* the same from host buffers (upload, compute, download) */
int mce_knn_dotp_part_f64(const double *Y, int64_t nr, int32_t d, int32_t kmax, int32_t part, int32_t nparts,
                          const double *w, const double *fs, double *dotp, int32_t device);

/* The ALL-PAIRS-ONCE partition of the same sums (round 5; optional -- parallel.py takes it when MCE_PAIRS_ONCE=1): where one GPU
 * would run the one-pass symmetric sweep (mce_pairs_once_blocks > 0), W ranks can multiply every pair of rows once per NODE
 * instead of once per side: rank r owns the sorted 512-row blocks r, r + W, ... and runs the single-GPU units of those blocks
 * (a block against every block below it, both gates on), and ships the candidates it found for rows it does not own to their owners.  Four calls on one workspace (sized as for
 * mce_knn_dotp_part_f64_dev), the collectives between them are the caller's (no RCCL dependency in this library):
 *   prepare -> *bounds_offset / *bounds_count: where in the workspace (bytes from its start) the rows' bounds lie -- doubles,
 *              +inf for the rows of other ranks: all-reduce them with MIN (every rank bounds the rows of its own blocks only);
 *   sweep   -> d_counts[nparts]: 16-byte candidates for every rank (own entry 0); d_flags[blocks]: blocks of other ranks whose
 *              candidates did not fit here (the owner searches such a block again: all-reduce the flags with MAX);
 *   export  -> d_send: the candidates, densely, ordered by destination rank (sum of d_counts entries of 16 bytes);
 *              exchange them (all_to_all with the counts as split sizes);
 *   finish  <- d_recv / nrecv: what arrived; d_flags: the reduced flags; -> d_dotp[kmax]: the sums over this rank's own rows
 *              (NaN if an entry arrived for a row the rank does not own: ranks that disagree about the partition).
 * Adding the nparts results gives mce_knn_dotp_f64_dev's dotp up to summation order.  Replaces the same reference lines as
 * mce_knn_dotp_f64_dev (MCEvidence.py:1093-1117) for one rank's rows. */
int32_t mce_pairs_once_blocks(int64_t nr, int32_t d, int32_t kmax);
/* the workspace of the three calls below (0: the partition does not exist for this shape): the search's and the reduction's, plus
 * one list set per chain of units when a rank's blocks are dealt to several chains (capi_apo.hpp: PairsOnceShape) */
size_t mce_pairs_once_workspace_bytes(int64_t nr, int32_t d, int32_t kmax, int32_t nparts);
int mce_pairs_once_prepare_dev(const double *dY, int64_t nr, int32_t d, int32_t kmax, int32_t part, int32_t nparts,
                               size_t *bounds_offset, int64_t *bounds_count, void *ws, size_t ws_bytes, void *stream);
int mce_pairs_once_sweep_dev(const double *dY, int64_t nr, int32_t d, int32_t kmax, int32_t part, int32_t nparts,
                             int64_t *d_counts, int32_t *d_flags, void *ws, size_t ws_bytes, void *stream);
int mce_pairs_once_export_dev(int64_t nr, int32_t d, int32_t kmax, int32_t part, int32_t nparts, void *d_send, void *ws,
                              size_t ws_bytes, void *stream);
int mce_pairs_once_finish_dev(const double *dY, int64_t nr, int32_t d, int32_t kmax, int32_t part, int32_t nparts,
                              const double *d_w, const double *d_fs, const void *d_recv, int64_t nrecv,
                              const int32_t *d_flags, double *d_dotp, void *ws, size_t ws_bytes, void *stream);

/* Name of the dominant kernel last launched by this thread and its launch
 * geometry (for bench.py / profiles): "knn_mfma_f64<KS=7,KCAP=12>" etc. */
const char *mce_last_kernel(void);
/* rows that the run-time certificate (mce_options.verify) of the most recent host-pointer search re-checked; 0: none ran */
int32_t mce_last_verify_rows(void);
/* SHA-256 (hex) of the kernel sources this library was built from (every .hpp and .hip file of csrc/ in name order; csrc/Makefile).
 * A committed rocprofv3 profile carries the same digest (profiles/<round>/meta.json): bench.py only quotes counters of a
 * profile that was taken from THESE sources. */
const char *mce_source_hash(void);

/* The host-pointer entry points keep their small device buffers (<= 64 MB each) in a per-thread
 * pool between calls; this frees them. */
void mce_release_device_memory(void);

/* Search algorithm.  0 (default) / 2: fp16-MFMA filter with exact fp64 refinement where the
 * shape allows it (all d <= 63, K <= 32), otherwise the fp64 MFMA sweep; 1: always the
 * fp64 MFMA sweep.  Both return the exact fp64 neighbours and distances.  Process-wide. */
int mce_set_search_mode(int mode);
int mce_get_search_mode(void);

/* Per-call options.  The three mode setters (this one, mce_set_prune_mode, mce_set_sym_mode) set PROCESS-WIDE DEFAULTS;
 * two threads with different needs would race on them.  A call carries its own modes instead:
 *   - the *_opt entry points below take a trailing `const mce_options*` (NULL: the defaults);
 *   - mce_options_push(&o) ... mce_options_pop() bracket any other entry point: the pushed modes apply to the calls THIS
 *     THREAD makes in between (they nest; threads the library starts itself, one per device, inherit them).
 * A mode of -1 means "the process default".  `size` = sizeof(mce_options) as the CALLER was built (room to grow): at least
 * 16 (size + the three modes); a field beyond `size` is never read and counts as -1. */
typedef struct mce_options {
    int32_t size;
    int32_t search_mode;   /* as mce_set_search_mode */
    int32_t prune_mode;    /* as mce_set_prune_mode  */
    int32_t sym_mode;      /* as mce_set_sym_mode    */
    int32_t same_set;      /* workspace queries: 1 = X and Y will be ONE buffer (auto evidence), 0 = they will not (no scratch
                              for the symmetric sweep is reserved: ~1.7 GB at 1 M rows, K = 9), -1 = unknown (reserved) */
    int32_t verify;        /* > 0: after the search, re-check this many query rows (spread over the set) by an independent exact
                              fp64 scan of ALL reference rows (mce_verify_knn_f64_dev below) and fail with MCE_ERR_VERIFY if a row
                              disagrees; honoured by the host-pointer entry points (mce_knn_f64[_opt], mce_knn_dotp_f64[_opt],
                              mce_evidence_feed[_batch]_f64 -- not by a rank's share, *_part_*) at d <= 128, K <= 32 (other shapes
                              run on exact fp64 kernels and are skipped silently).  0: off.  -1 (the default, round 6): a search
                              that went through the fp16 FILTER is re-checked on 256 rows -- every call from 65 536 query rows
                              on, one call in eight of the smaller ones (there the check is launch overhead, not rows: 0.16 of
                              0.68 ms at 7 k x 6) -- and one on the fp64 kernels is not; MCE_VERIFY=n in the environment: n rows
                              on EVERY call; MCE_VERIFY=0: off.  ~1 ms at 1 M x 27 with the distances it needs written out */
    int32_t eig_mode;      /* evidence feed (mce_evidence_feed_f64, _batch[_dev], _part[_dev], _whiten[_dev], _prefix[_dev]): who solves the
                              covariance eigen-system.  0 (what every caller built before this field sends: it was reserved[0]): the
                              process default -- MCE_FEED_EIG=host|hip in the environment, read once; host when unset.  1: the host
                              (one core, between two waits).  2: the device (mce_eig_sym_batch_dev_f64 on the call's stream; the
                              call waits once, a batch once per wave).  The two agree within C eps cond(Cn) per eigenvalue, not bit
                              for bit (docs/design/device_eig.md) */
    int32_t reserved[1];   /* 0 */
} mce_options;
#define MCE_EIG_DEFAULT 0
#define MCE_EIG_HOST 1
#define MCE_EIG_DEVICE 2
int mce_options_push(const mce_options* opt);
int mce_options_pop(void);
int mce_knn_f64_opt(const double* X, int64_t nq, const double* Y, int64_t nr, int32_t d, int32_t K, int32_t self_mode,
                    int64_t self_offset, double* dist, int64_t* idx, int32_t device, const mce_options* opt);
int mce_knn_dotp_f64_opt(const double* X, int64_t nq, const double* Y, int64_t nr, int32_t d, int32_t kmax, int32_t k0,
                         int64_t self_offset, const double* w, const double* fs, double* dotp, double* dist_out,
                         const int32_t* devices, int32_t ndev, const mce_options* opt);
int mce_knn_dotp_f64_dev_opt(const double* dX, int64_t nq, const double* dY, int64_t nr, int32_t d, int32_t kmax, int32_t k0,
                             int64_t self_offset, const double* d_w, const double* d_fs, double* d_dotp, double* d_dist_out,
                             void* ws, size_t ws_bytes, void* stream, const mce_options* opt);
size_t mce_knn_workspace_bytes_opt(int64_t nq, int64_t nr, int32_t d, int32_t K, const mce_options* opt);

/* Batched symmetric eigen-solver (the feed's, d <= 127): `nsys` row-major symmetric d x d matrices cov[nsys][d*d] -> evec[nsys][d*d]
 * (eigenvectors in the COLUMNS, each one's first largest-magnitude component positive), scale[nsys][d] = 1 / sqrt(lam),
 * lam[nsys][d] (descending, ties in the order of a stable sort) and status[nsys][MCE_EIG_STATUS_INTS] = {code, index, sweeps,
 * rotations}: code 0 ok; 1 the matrix holds a NaN or an infinity (no sweep runs); 2 eigenvalue `index` is not > 0.  A system whose
 * code is not 0 fails alone and still gets finite evec (the identity) and scale (1).
 *   _dev: device pointers, one workgroup per system (parallel Jacobi in a round-robin tournament order, the whole matrix in LDS),
 *         enqueued on `stream`, never synchronises.  A system's bits depend on its own matrix alone.
 *   host pointers: `mode` MCE_EIG_HOST runs the feed's host solver (cyclic Jacobi; sweeps and rotations are reported as 0),
 *         MCE_EIG_DEVICE uploads, runs the kernel on `device` and copies back.
 * mce_last_eig_stats: out[4] = for the calling thread's last evidence-feed call, systems solved on the device, systems solved on the
 * host, the largest number of sweeps and the rotations in all (device solves only). */
#define MCE_EIG_STATUS_INTS 4
int mce_eig_sym_batch_dev_f64(const double* d_cov, int32_t d, int64_t nsys, double* d_evec, double* d_scale, double* d_lam, int32_t* d_status,
                              void* stream);
int mce_eig_sym_batch_f64(const double* cov, int32_t d, int64_t nsys, int32_t mode, double* evec, double* scale, double* lam, int32_t* status,
                          int32_t device);
int mce_last_eig_stats(double* out, int32_t n);

/* Run-time certificate of a finished search (reference: the result of `nbrs.kneighbors(samples)`, MCEvidence.py:1104, whose
 * exactness everything downstream rests on).  For `nsample` query rows spread evenly over the set (sample s of n = min(nsample,
 * nq) is row (seed % nq + floor(s nq / n)) % nq: n distinct rows, no cyclic gap between them above ceil(nq / n)) every reference
 * row's squared distance is recomputed by plain fp64 differences -- none of the search's machinery:
 * no matrix cores, no packed operands, no bounds, no lists -- and counted against the K distances the search reported for
 * that row (`dist`, [nq][ld] as mce_knn_f64 / dist_out write them): nobody outside the list may be closer than its k-th
 * entry, and at least k rows must lie within it (relative tolerance 1e-9 on the squared distance).  d <= 128, K <= 32.
 * An entry that is no distance fails its row: NaN, a negative number, and +inf in column k (counted from 1) unless fewer than k
 * usable reference rows exist (the own row is not usable under MCE_SELF_EXCLUDE) -- the one case in which a search has nothing to
 * report there; an entry point of this library refuses K > usable rows, so its lists never hold one.
 * _dev: device pointers, the caller's stream, never synchronises; `d_result` (device, 2 ints) receives {rows checked, rows
 * that failed}; workspace from mce_verify_workspace_bytes.  The host-pointer form uploads, checks, and returns
 * MCE_ERR_VERIFY (message: how many rows failed) or MCE_OK; `failed` (optional) receives the count. */
size_t mce_verify_workspace_bytes(int32_t nsample, int32_t K);
int mce_verify_knn_f64_dev(const double* dX, int64_t nq, const double* dY, int64_t nr, int32_t d, int32_t K, int32_t self_mode,
                           int64_t self_offset, const double* d_dist, int32_t ld, int32_t nsample, uint64_t seed, int32_t* d_result,
                           void* ws, size_t ws_bytes, void* stream);
int mce_verify_knn_f64(const double* X, int64_t nq, const double* Y, int64_t nr, int32_t d, int32_t K, int32_t self_mode,
                       int64_t self_offset, const double* dist, int32_t ld, int32_t nsample, uint64_t seed, int32_t* failed,
                       int32_t device);

/* Chain text -> fp64 on the device: what mce_chain_open / _read of libmcechains.so (include/mcechains.h) return for the same bytes,
 * bit for bit (replaces np.loadtxt at reference MCEvidence.py:564).  Fields separated by ' ', \t, \v, \f; '#' starts a comment that
 * runs to the end of the line; \n and \r both end a line; blank and comment-only lines are skipped; every data line must hold the
 * fields of the first one.  open uploads `text` (host memory, e.g. a mapping of the file; it must stay valid until close) and finds
 * rows and columns; read converts every field on the device -- one correctly rounded IEEE operation for up to 15 digits, the
 * Eisel-Lemire scheme for up to 19 -- and patches what the device cannot decide (inf, nan, longer tails, subnormals, junk) with the
 * host's strtod.  A ragged file (open) or a field that is not a number (read) -> MCE_ERR_INVALID; no visible device ->
 * MCE_ERR_NO_DEVICE; a failed device allocation -> MCE_ERR_HIP.  A handle belongs to one thread; several may be open on one device.
 *   out: host, [nrows * ncols] row-major.  stats (may be NULL, nstats >= 6): {tokens, tokens patched on the host, ms upload,
 *   ms structure, ms parse, ms download} */
int mce_chain_dev_open(const char* text, int64_t nbytes, int32_t device, void** handle, int64_t* nrows, int64_t* ncols);
int mce_chain_dev_read(void* handle, double* out, double* stats, int32_t nstats);
void mce_chain_dev_close(void* handle);
/* mce_chain_dev_read with the values left ON THE DEVICE: d_out is a device buffer of nrows * ncols doubles on the handle's device.
 * The tokens the device leaves undecided are converted by the host's strtod from the caller's text, as in mce_chain_dev_read, and
 * written to d_out in one small copy (stats[5], "ms download", is that copy); a field that is not a number fails with the same
 * message.  The handle's stream is synchronised on return. */
int mce_chain_dev_read_dev(void* handle, double* d_out, double* stats, int32_t nstats);

/* Burn-in, concatenation, thinning, the s1 / s2 split, the column split and the fs / SumW reductions of chains that are on the device
 * already (replaces the host passes of reference MCEvidence.py:350-391 removeBurn, :447-532 thinning, :221-249 the split, :394-405 the
 * column split and :1062-1064 fs).  A chain is a list of parts -- device buffers [nrows, ncols] of doubles, one per file, the
 * burn-in already skipped by the caller (pointer + start * ncols; the start is mce_prep::burn_start of csrc/chain_prep.hpp) -- whose
 * rows are numbered consecutively ("burned, concatenated numbering").  All buffers and workspaces are the caller's, on the current
 * device; everything runs on `stream`.  Argument errors: MCE_ERR_INVALID (no device needed); no visible device: MCE_ERR_NO_DEVICE.
 *   weights       gathers the weight column and its int64 prefix sums into the workspace; totals[5] = {rows, sum of trunc(w), max of
 *                 trunc(w), sum of w - trunc(w), weights that are negative / not finite / beyond 2^53}; *rule = 0 no thinning
 *                 (thinlen 0 or 1), 1 integer-weight rule, 2 bin rule, < 0 the route must decline: -1 a refused weight, -2 the
 *                 fractional sum lies within 1e-6 of the host's threshold 1e-4, -3 thinlen < 0 or 0 < thinlen < 1.
 *   select_count  (same workspace) *n_out = rows the rule keeps; d_edges[nedges]: np.linspace(-1, n, nbins + 1) computed on the host
 *                 (bin rule only; NULL otherwise).
 *   select_fill   (same workspace) d_src[n_out]: the kept rows in the burned, concatenated numbering -- the host's `keep`, rows may
 *                 repeat --, d_new_w[n_out]: their new weights.
 *   gather        output row r is row (d_src ? d_src[k] : k), k = d_rows ? d_rows[r] : r (d_rows: an index list into the n_thin
 *                 thinned rows, e.g. one side of a split).  Any of: d_params [n_out, ncols - itheta], d_w [n_out] (d_new_w[k] if
 *                 given, else column iw), d_like [n_out] (column ilike), d_full [n_out, ncols] (the thinned rows, weight replaced).
 *                 Synchronises the stream.
 *   reduce        d_fs[n] = logL - max(logL), logL = pos_lnp ? d_like : -d_like; out[4] (host) = {max(logL) over the rows that are
 *                 not NaN, SumW = sum of d_w, NaN likelihoods, weights that are not finite}.  Sums in a fixed order: two runs give
 *                 the same bits.  Synchronises the stream. */
typedef struct mce_chain_part {
    const double* rows;
    int64_t nrows;
} mce_chain_part;
size_t mce_chain_select_workspace_bytes(int64_t n, int32_t nparts);
size_t mce_chain_gather_workspace_bytes(int32_t nparts);
size_t mce_chain_reduce_workspace_bytes(int64_t n);
int mce_chain_weights_dev(const mce_chain_part* parts, int32_t nparts, int64_t ncols, int32_t iw, double thinlen, int32_t* rule,
                          double* totals, void* ws, size_t ws_bytes, void* stream);
int mce_chain_select_count_dev(int64_t n, int32_t nparts, int32_t rule, double thinlen, const double* d_edges, int64_t nedges,
                               int64_t* n_out, void* ws, size_t ws_bytes, void* stream);
int mce_chain_select_fill_dev(int64_t n, int32_t nparts, int32_t rule, double thinlen, int64_t nedges, int64_t n_out, int64_t* d_src,
                              double* d_new_w, void* ws, size_t ws_bytes, void* stream);
int mce_chain_gather_dev(const mce_chain_part* parts, int32_t nparts, int64_t ncols, int32_t iw, int32_t ilike, int32_t itheta,
                         const int64_t* d_src, const double* d_new_w, int64_t n_thin, const int64_t* d_rows, int64_t n_out,
                         double* d_params, double* d_w, double* d_like, double* d_full, void* ws, size_t ws_bytes, void* stream);
int mce_chain_reduce_dev(const double* d_like, const double* d_w, int64_t n, int32_t pos_lnp, double* d_fs, double* out, void* ws,
                         size_t ws_bytes, void* stream);

/* The autocorrelation length of burned chains that are on the device, and with it the thinning factor of thin_corr (the reference's
 * command line promises "thinlen < 0: the autocorrelation length of the chain" and raises; here the length is measured under its own
 * keyword).  The rule is stated in csrc/chain_corr.hpp and docs/design/chain_corr.md: the series of a part is its rows repeated
 * trunc(w) times (integer weights: *rule = 1, weight units) or the rows themselves (*rule = 2, row units), the rule being
 * mce_chain_weights_dev's verdict for thinlen = 2; *rule < 0 is that call's decline and nothing else is set.  The first `ndim`
 * columns from `itheta` are measured (1 <= ndim <= 127): per column the pooled lagged sums S_j(t) over the parts -- a pair never
 * spans two parts --, rho_j(t), cut[j] = the first t in 1 .. cap with rho_j(t) <= min_corr (0 <= min_corr < 1) and
 * length[j] = 1 + 2 sum_{t < cut[j]} rho_j(t); *cap = min(max_lag, largest part's units / 4), max_lag in 1 .. 65536; *units = the
 * units of all parts.  status[0]: 0 ok, 1 some column has no cut within the cap, 2 a column with S_j(0) not > 0 (constant), 3 a value
 * that is not finite in a measured column; status[1] = that column.  length / cut of a column without a cut: the sum so far and 0.
 * rho (host, may be NULL): rho[t * ndim + j] for t < *rho_rows, the lags that were summed (the windows stop after the one in which the
 * last column found its cut); later rows of the table are left untouched.  fp64, sums in a fixed order: two runs give the same bits.
 * Parts, workspace and stream are the caller's (mce_chain_corr_workspace_bytes(rows of all parts, nparts, ndim, max_lag)); the stream
 * is synchronised on return.  mce_chain_corr_f64 takes HOST parts, uploads them to `device` and calls the device form.
 * Argument errors: MCE_ERR_INVALID (no device needed); no visible device: MCE_ERR_NO_DEVICE. */
size_t mce_chain_corr_workspace_bytes(int64_t n, int32_t nparts, int32_t ndim, int64_t max_lag);
int mce_chain_corr_dev(const mce_chain_part* parts, int32_t nparts, int64_t ncols, int32_t iw, int32_t itheta, int32_t ndim, double min_corr,
                       int64_t max_lag, int32_t* rule, int32_t* status, int64_t* units, int64_t* cap, double* length, int64_t* cut,
                       double* rho, int64_t* rho_rows, void* ws, size_t ws_bytes, void* stream);
int mce_chain_corr_f64(const mce_chain_part* parts, int32_t nparts, int64_t ncols, int32_t iw, int32_t itheta, int32_t ndim, double min_corr,
                       int64_t max_lag, int32_t* rule, int32_t* status, int64_t* units, int64_t* cap, double* length, int64_t* cut,
                       double* rho, int64_t* rho_rows, int32_t device);

/* Delete-a-group jackknife of the evidence reduction from ONE neighbour search (docs/design/jackknife.md; rule: csrc/jack.hpp).
 * Every query row q has an ascending list of L entries, d_dist / d_idx [nq][L] (what mce_knn_f64_dev leaves; a row below 0 ends the
 * list), a weight, a term fs and a group d_gq[q] in [0, G); every reference row has a group d_gr[nr].  With K = kmax - k0:
 *   d_dotp_groups[b * kmax + k] = the sum mce_dotp_f64_dev forms for column k, over the rows with d_gq != b, each taken at the
 *                                 (k - k0 + 1)-th entry of its list once entries whose reference row is in group b are skipped;
 *   d_dotp_full[k]              = the same with no group deleted (with no short row: mce_dotp_f64_dev's sum, bit for bit).
 * k0 = 1 (auto evidence): the entry whose reference row is the query's own -- d_qid[q], or q where d_qid is NULL -- is skipped too.
 * A row is SHORT when skipping some group other than its own (or none) leaves fewer than K entries: it enters no sum; its row
 * number (d_qid[q] or q) is appended to d_short_rows [nq], ascending, and *d_nshort (device) counts them.  d_gq, d_w, d_fs are
 * indexed by q, not by d_qid.  2 <= G <= MCE_JACK_MAX_GROUPS, K <= L <= MCE_GENERIC_MAX_K + 1, K <= MCE_MAX_K.  Lists of up to 32
 * entries are processed from registers, longer ones from memory.  fp64, plain stores, sums in an order the sizes fix: two runs give
 * the same bits.  The stream is synchronised on return.  mce_jack_dotp_f64 takes HOST pointers (nshort too), uploads to `device`
 * and calls the device form.  Argument errors -- G out of range, a group id out of range, L < K -- : MCE_ERR_INVALID. */
#define MCE_JACK_MAX_GROUPS 64
size_t mce_jack_workspace_bytes(int64_t nq, int32_t G, int32_t kmax);
int mce_jack_dotp_dev(const double* d_dist, const int64_t* d_idx, int64_t nq, int32_t L, const int64_t* d_qid, const int32_t* d_gq,
                      const int32_t* d_gr, int64_t nr, int32_t G, int32_t k0, int32_t kmax, int32_t d, const double* d_w, const double* d_fs,
                      double* d_dotp_groups, double* d_dotp_full, int64_t* d_short_rows, int64_t* d_nshort, void* ws, size_t ws_bytes,
                      void* stream);
int mce_jack_dotp_f64(const double* dist, const int64_t* idx, int64_t nq, int32_t L, const int64_t* qid, const int32_t* gq, const int32_t* gr,
                      int64_t nr, int32_t G, int32_t k0, int32_t kmax, int32_t d, const double* w, const double* fs, double* dotp_groups,
                      double* dotp_full, int64_t* short_rows, int64_t* nshort, int32_t device);

/* The k-NN relative entropy D_KL(P || Q) of two weighted samples with a delete-a-group jackknife from ONE pair of neighbour searches
 * (docs/design/knn_divergence.md; rule: csrc/knn_div.hpp).
 *
 * mce_div_whiten_dev: z[n][d] (packed: what mce_knn_f64_dev reads) = linv (x - mean) for the rows d_x[n][ld] on the device; linv[d * d]
 * (lower triangle, row major) and mean[d] are HOST arrays and travel with the call; the products of a coordinate are added in column
 * order.  report[MCE_DIV_REPORT] (HOST): the sum of d_w, the count of weights that are not > 0 or not finite, the lowest column with a
 * value that is not finite (-1: none), n -- summed in an order the sizes fix.  1 <= d <= MCE_DIV_MAX_DIM.  The stream is synchronised on
 * return.  Workspace: mce_div_whiten_workspace_bytes(n, d).
 *
 * mce_knn_div_terms_dev: every query row q (a row of P: d_qid[q], or q where d_qid is NULL) has two ascending lists of L entries, the
 * AUTO list d_distP / d_idxP [nq][L] (its neighbours in P; an entry whose row is the query's own is skipped) and the CROSS list
 * d_distQ / d_idxQ [nq][L] (its neighbours in Q); a row below 0 ends a list.  d_gq[nq], d_grP[nP], d_grQ[nQ]: groups in [0, G);
 * d_aq[nq], d_aP[nP], d_bQ[nQ]: weights.  d_sums[(G + 1)][K][2]: slot 0 the full sample, slot 1 + b with group b deleted from both
 * samples; per rank k the sums N and X of the rule.  The weight of P and of its groups is formed inside the call.  A row is SHORT when
 * skipping some group other than its own (or none) leaves fewer than K entries in either list: it enters no sum; its row number is
 * appended to d_short_rows [nq], ascending, and *d_nshort (device) counts them.  G = 0: no groups (the group pointers may be NULL), the
 * full slot alone.  Otherwise 2 <= G <= MCE_JACK_MAX_GROUPS.  K <= L <= MCE_GENERIC_MAX_K; K > MCE_DIV_MAX_K: MCE_ERR_K_RANGE.  Lists of
 * up to 32 entries are processed from registers, longer ones from memory.  fp64, plain stores, sums in an order the sizes fix: two runs
 * give the same bits.  The stream is synchronised on return.  The *_f64 forms take HOST pointers (nshort too), upload to `device` and
 * call the device forms.  Argument errors -- G out of range, a group id out of range, L < K -- : MCE_ERR_INVALID. */
#define MCE_DIV_MAX_K 16
#define MCE_DIV_MAX_DIM 64
#define MCE_DIV_REPORT 4
size_t mce_div_whiten_workspace_bytes(int64_t n, int32_t d);
int mce_div_whiten_dev(const double* d_x, int64_t ld, int64_t n, int32_t d, const double* linv, const double* mean, const double* d_w, double* d_z,
                       double* report, void* ws, size_t ws_bytes, void* stream);
int mce_div_whiten_f64(const double* x, int64_t ld, int64_t n, int32_t d, const double* linv, const double* mean, const double* w, double* z,
                       double* report, int32_t device);
size_t mce_knn_div_workspace_bytes(int64_t nq, int64_t nP, int32_t G, int32_t K);
int mce_knn_div_terms_dev(const double* d_distP, const int64_t* d_idxP, const double* d_distQ, const int64_t* d_idxQ, int64_t nq, int32_t L,
                          const int64_t* d_qid, const int32_t* d_gq, const int32_t* d_grP, int64_t nP, const int32_t* d_grQ, int64_t nQ, int32_t G,
                          int32_t K, int32_t d, const double* d_aq, const double* d_aP, const double* d_bQ, double* d_sums, int64_t* d_short_rows,
                          int64_t* d_nshort, void* ws, size_t ws_bytes, void* stream);
int mce_knn_div_terms_f64(const double* distP, const int64_t* idxP, const double* distQ, const int64_t* idxQ, int64_t nq, int32_t L, const int64_t* qid,
                          const int32_t* gq, const int32_t* grP, int64_t nP, const int32_t* grQ, int64_t nQ, int32_t G, int32_t K, int32_t d,
                          const double* aq, const double* aP, const double* bQ, double* sums, int64_t* short_rows, int64_t* nshort, int32_t device);

/* The bookkeeping of the delete-a-group jackknife for chains that stay on the device (the resident route and the farm;
 * docs/design/jackknife_resident.md; rule: csrc/jack_groups.hpp), for MANY systems (the asking roots of a farm wave) in one call.
 *
 * mce_jack_groups_dev: the group of every row.  Row i of a segment is sample row r = rows[i] (rows NULL: r = i) of a burned,
 * concatenated, thinned sample of N rows.  by = MCE_JACK_BY_BLOCKS: out[i] = r * G / N in 64-bit integers.  by = MCE_JACK_BY_CHAINS:
 * s = src[r] (src NULL: s = r) is the row's number in the burned, concatenated numbering and out[i] = the last part p with
 * part_first[p] <= s; part_first is a HOST array of nparts == G non-decreasing first rows starting at 0 (an empty part shares its first
 * row with the next one and is never the answer).  rows [n], src [N] and out [n] are DEVICE pointers.  An r outside [0, N) gives -1,
 * which mce_jack_dotp_dev and mce_jack_leave_out_dev refuse.  One launch whatever nseg is; the stream is synchronised on return.
 *
 * mce_jack_leave_out_dev: one block of MCE_JACK_LEAVE_OUT doubles per slot of every system, packed in segment order: system s owns
 * G_s + 1 consecutive blocks, slot 0 with nothing deleted and slot 1 + b with group b deleted, each taken over the rows with g != b:
 * {rows (zero-weight rows count), SumW = sum w, and mce_like_moments_dev's block on that set: W, c, v about the slot's own computed c,
 * A2, rows used, status}.  fs NULL: the six moment values are NaN and the status is -1.  Status 0 / 3 / 5 and NaN as in
 * mce_like_moments_dev; a slot that fails does so alone.  Every sum is a sum of the set's own terms (additions only, never total -
 * group), fp64, in an order the system's row count fixes: two runs give the same bits and a system's bits depend on its own rows
 * alone.  Four launches whatever nseg is, all on the caller's stream, which is synchronised once, on return.  Segments and workspace
 * (mce_jack_leave_out_workspace_bytes(rows of all segments, nseg, the largest G)) are the caller's.  mce_jack_leave_out_f64 takes HOST
 * segments, uploads them to `device` and calls the device form.  Argument errors -- G outside 2 .. MCE_JACK_MAX_GROUPS, a group id
 * outside [0, G) -- : MCE_ERR_INVALID; no visible device: MCE_ERR_NO_DEVICE. */
#define MCE_JACK_LEAVE_OUT 8
#define MCE_JACK_BY_BLOCKS 0
#define MCE_JACK_BY_CHAINS 1
typedef struct mce_jack_groups_seg {
    const int64_t* rows;
    const int64_t* src;
    const int64_t* part_first;
    int64_t nparts;
    int64_t n;
    int64_t N;
    int32_t G;
    int32_t by;
    int32_t* out;
} mce_jack_groups_seg;
typedef struct mce_jack_leave_out_seg {
    const double* w;
    const double* fs;
    const int32_t* g;
    int64_t n;
    int32_t G;
} mce_jack_leave_out_seg;
int mce_jack_groups_dev(const mce_jack_groups_seg* segs, int32_t nseg, void* stream);
size_t mce_jack_leave_out_workspace_bytes(int64_t nrows_total, int32_t nseg, int32_t Gmax);
int mce_jack_leave_out_dev(const mce_jack_leave_out_seg* segs, int32_t nseg, double* out, void* ws, size_t ws_bytes, void* stream);
int mce_jack_leave_out_f64(const mce_jack_leave_out_seg* segs, int32_t nseg, double* out, int32_t device);

/* The Gelman-Rubin statistic "R-1" of burned chains that are on the device, for MANY systems (the roots of a farm wave) in one call:
 * the variance of the chain means over the mean of the chain variances, in the worst direction of parameter space.  The rule is stated
 * in csrc/chain_conv.hpp and docs/design/chain_conv.md.  `segs` are runs of rows of `ncols` doubles (a whole chain, or a half of one: a
 * segment whose pointer is offset -- halves are the caller's business); seg_sys[s] in 0 .. nsys - 1, non-decreasing, names the system
 * of segment s; a system has at most MCE_CONV_MAX_SEGMENTS segments.  The RAW weights of column `iw` weigh the first `ndim` columns
 * from `itheta` (1 <= ndim <= 127); one call takes one (ncols, ndim).  A segment without rows or of total weight 0 is skipped;
 * nseg_used[y] counts the others.  Outputs are HOST arrays: r_minus_1[nsys], per_param[nsys * ndim] (B_jj / W_jj), status[2 * y] =
 * 0 ok, 2 a column whose within-chain variance is not > 0 (constant), 3 a value that is not finite in a measured column or a weight
 * that is negative or not finite, 4 the within-chain correlation matrix is not positive definite (per_param is still set, r_minus_1
 * is NaN), 5 fewer than two segments with weight; status[2 * y + 1] = the offending column (-1: a weight, or none).  Where the status is
 * 2, 3 or 5, r_minus_1 and per_param are NaN.  A system's bits depend on its own rows alone, not on its neighbours, its position or
 * the call; fp64, sums in a fixed order: two runs give the same bits.  Segments, workspace and stream are the caller's
 * (mce_chain_conv_workspace_bytes(rows of all segments, nseg, nsys, ndim)); everything is enqueued on the stream, which is
 * synchronised once, on return.  mce_chain_conv_f64 takes HOST segments, uploads them to `device` and calls the device form.
 * Argument errors: MCE_ERR_INVALID (no device needed) -- ndim outside 1 .. 127, more than MCE_CONV_MAX_SEGMENTS segments in a system,
 * a system with fewer than 2 segments with rows, seg_sys out of order; no visible device: MCE_ERR_NO_DEVICE. */
#define MCE_CONV_MAX_SEGMENTS 128
size_t mce_chain_conv_workspace_bytes(int64_t nrows_total, int32_t nseg, int32_t nsys, int32_t ndim);
int mce_chain_conv_dev(const mce_chain_part* segs, const int32_t* seg_sys, int32_t nseg, int32_t nsys, int64_t ncols, int32_t iw, int32_t itheta,
                       int32_t ndim, double* r_minus_1, double* per_param, int32_t* status, int32_t* nseg_used, void* ws, size_t ws_bytes,
                       void* stream);
int mce_chain_conv_f64(const mce_chain_part* segs, const int32_t* seg_sys, int32_t nseg, int32_t nsys, int64_t ncols, int32_t iw, int32_t itheta,
                       int32_t ndim, double* r_minus_1, double* per_param, int32_t* status, int32_t* nseg_used, int32_t device);

/* The weighted moments of the likelihood column behind information= (<ln L>_P, the Bayesian model dimensionality 2 Var_P(ln L), N_eff),
 * for MANY systems (the ready roots of a farm wave) in one call.  The rule is stated in csrc/like_moments.hpp and
 * docs/design/information.md.  A system is one segment: fs[n] = logL - logLmax and w[n], the weights, of the s1 partition the estimator
 * sums over; a row with w == 0 is skipped and its fs never read into a sum.  out (HOST, MCE_MOMENTS_OUT doubles per system) =
 * {W = sum w, c = sum w fs / W, v = sum w (fs - c)^2 / W about the computed c, A2 = sum w^2, rows used, status}; status 0 ok, 3 a weight
 * that is not finite or a used row whose fs is not finite (-inf included), 5 W is not > 0 (a segment without a used row included); where
 * the status is not 0 the four values are NaN, and that system fails alone.  A system's bits depend on its own rows alone, not on its
 * neighbours, its position or the call; fp64, sums in a fixed order, no atomics: two runs give the same bits.  Four launches whatever
 * nseg is, all on the caller's stream, which is synchronised once, on return.  Segments and workspace
 * (mce_like_moments_workspace_bytes(rows of all segments, nseg)) are the caller's.  mce_like_moments_f64 takes HOST segments, uploads
 * them to `device` and calls the device form.  Argument errors: MCE_ERR_INVALID (no device needed); no visible device:
 * MCE_ERR_NO_DEVICE. */
#define MCE_MOMENTS_OUT 6
typedef struct mce_moments_seg {
    const double* fs;
    const double* w;
    int64_t n;
} mce_moments_seg;
size_t mce_like_moments_workspace_bytes(int64_t nrows_total, int32_t nseg);
int mce_like_moments_dev(const mce_moments_seg* segs, int32_t nseg, double* out, void* ws, size_t ws_bytes, void* stream);
int mce_like_moments_f64(const mce_moments_seg* segs, int32_t nseg, double* out, int32_t device);

/* The posterior summary behind summary= (weighted mean, variance, extremes, weighted quantiles and the best-fit sample of the first d
 * parameter columns), for MANY systems (the ready roots of a farm wave) in one call.  The rule is stated in csrc/param_summary.hpp and
 * docs/design/summary.md.  One system is one segment: x[n][ld] the RAW rows (the first d columns are measured), w[n] the weights and
 * fs[n] = logL - logLmax of the s1 partition the estimator sums over; segments may differ in d and ld.  A row with w == 0 is skipped
 * and nothing of it is read into a result.  q[nq]: the targets, each in (0, 1); Q_j(q) is the smallest value of column j among the used
 * rows whose cumulative weight reaches q W (no interpolation).  out (HOST, packed in segment order, mce_param_summary_out_doubles(d, nq)
 * doubles per system) = {W, A2 = sum w^2, rows used, status, column, best-fit row, best-fit f, reserved} then mean[d], var[d] (about the
 * computed mean), min[d], max[d], bestfit[d] and nq rows of quantiles [d].  status 0 ok (column -1); 3 a weight that is negative or not
 * finite (column -1), else a used row whose f is NaN (column -2), else a used row with a value that is not finite (column: the lowest
 * such); 5 W is not > 0 (a segment without a used row included).  Where the status is not 0 every value is NaN, the best-fit row -1, and
 * that system fails alone.  fs == NULL: the best-fit entries are NaN / -1 and nothing else changes.  pass_elems: 0 for
 * MCE_SUMMARY_PASS_ELEMS, or the largest number of (row, column) elements sorted in one pass; a column longer than that is a pass of
 * its own.  A system's bits depend on its own rows alone, not on its neighbours, its position, the call or pass_elems; two runs give the
 * same bits; fp64, sums in a fixed order, no floating-point atomics, plain stores, 64-bit row indices.  The number of launches depends on
 * the number of passes, not on nseg; everything runs on the caller's stream, which this library synchronises once, on return.  One
 * caveat: the sort of a pass is rocprim::segmented_radix_sort_pairs, and from its partitioning threshold of runs in a pass on (3 000 in
 * its default configuration; a farm wave of 24 roots of 27 columns has 648) rocPRIM itself reads two segment counts back and waits
 * for the stream before it sorts: one more host wait per such pass, inside the call.  Segments and workspace
 * (mce_param_summary_workspace_bytes(rows of all segments, the longest segment, nseg, the largest d, nq, pass_elems)) are the caller's.
 * The size holds on the host and for the device it was asked on: it includes rocPRIM's temporary, which is asked of rocPRIM for the
 * largest pass and the largest number of runs the arguments allow (on the assumption that it does not shrink when either grows) where
 * a device is visible, and is an estimate where none is -- a size formed without a device is for planning only and must not be
 * carried to another host.  The device form asks rocPRIM again for every pass and returns MCE_ERR_WORKSPACE, before it sorts, if that
 * pass needs more than was planned.  mce_param_summary_f64 takes HOST segments, uploads them to `device` and calls the device form.  Argument errors (d outside
 * 1 .. 127, nq outside 1 .. MCE_SUMMARY_MAX_Q, a q outside (0, 1), ld < d, negative sizes): MCE_ERR_INVALID (no device needed); no visible
 * device: MCE_ERR_NO_DEVICE. */
#define MCE_SUMMARY_MAX_Q 16
#define MCE_SUMMARY_HEAD 8
#define MCE_SUMMARY_PASS_ELEMS (1 << 25)
typedef struct mce_summary_seg {
    const double* x;
    int64_t ld;
    int64_t n;
    int32_t d;
    const double* w;
    const double* fs;
} mce_summary_seg;
size_t mce_param_summary_out_doubles(int32_t d, int32_t nq);
size_t mce_param_summary_workspace_bytes(int64_t nrows_total, int64_t nrows_max, int32_t nseg, int32_t dmax, int32_t nq, int64_t pass_elems);
int mce_param_summary_dev(const mce_summary_seg* segs, int32_t nseg, const double* q, int32_t nq, int64_t pass_elems, double* out, void* ws, size_t ws_bytes,
                          void* stream);
int mce_param_summary_f64(const mce_summary_seg* segs, int32_t nseg, const double* q, int32_t nq, int64_t pass_elems, double* out, int32_t device);

/* The weighted parameter covariance behind covariance= (the weighted mean and the covariance matrix of the first d parameter columns),
 * for MANY systems (the ready roots of a farm wave) in one call.  The rule is stated in csrc/param_cov.hpp and docs/design/tension.md.
 * One system is one segment: x[n][ld] the RAW rows (the first d columns are measured) and w[n] the weights of the s1 partition the
 * estimator sums over; segments may differ in d and ld.  A row with w == 0 is skipped and nothing of it is read into a result.
 * out (HOST, packed in segment order, mce_param_cov_out_doubles(d) doubles per system) = {W, A2 = sum w^2, rows used, status, column,
 * reserved x 3} then mean[d] (bit for bit mce_param_summary_dev's mean of the same segment) and cov[d (d + 1) / 2], the packed upper
 * triangle, row-major, i <= j: C_ij = sum w (x_i - m_i)(x_j - m_j) / W about the computed mean.  status 0 ok (column -1); 3 a weight
 * that is negative or not finite (column -1), else a used row with a value that is not finite (column: the lowest such); 5 W is not
 * > 0.  With a status other than 0 every value is NaN; a failing system fails alone.  A system's bits depend on its own rows alone:
 * not on its neighbours, its position or the number of systems.  Everything runs on `stream` with one host wait; the number of
 * launches does not depend on nseg.  Segments and workspace (mce_param_cov_workspace_bytes(rows of all segments, nseg, the largest d))
 * are the caller's.  mce_param_cov_f64 takes HOST segments, uploads them to `device` and calls the device form.  Argument errors (d
 * outside 1 .. 127, ld < d, negative sizes, null pointers): MCE_ERR_INVALID (no device needed); no visible device: MCE_ERR_NO_DEVICE. */
#define MCE_COV_HEAD 8
typedef struct mce_cov_seg {
    const double* x;
    int64_t ld;
    int64_t n;
    int32_t d;
    const double* w;
} mce_cov_seg;
size_t mce_param_cov_out_doubles(int32_t d);
size_t mce_param_cov_workspace_bytes(int64_t nrows_total, int32_t nseg, int32_t dmax);
int mce_param_cov_dev(const mce_cov_seg* segs, int32_t nseg, double* out, void* ws, size_t ws_bytes, void* stream);
int mce_param_cov_f64(const mce_cov_seg* segs, int32_t nseg, double* out, int32_t device);

/* The non-Gaussian parameter shift behind shift="kde" (--shift-kde): a leave-one-out Gaussian kernel density estimate on the whitened rows
 * of a parameter-DIFFERENCE chain, and the weight of the rows whose density lies above the density at a point, for MANY systems in one
 * call.  The rule is stated in csrc/kde_shift.hpp and docs/design/shift_kde.md.  One system is one segment: x[n][ld] the rows (the first
 * d columns are measured, 1 <= d <= MCE_KDE_MAX_DIM) and w[n] their weights, on the DEVICE (mce_kde_shift_f64: on the host); linv[d * d]
 * (row-major, the lower triangle of the inverse Cholesky factor of the rows' covariance; what lies above the diagonal is not read),
 * mean[d] and point[d] are HOST arrays in both forms; c = 1 / (2 h^2) > 0.  z = linv (x - mean);  for a used row i,
 * S_i = sum over used j != i of w_j exp(-c max(0, |z_i - z_j|^2)) and t_i = S_i / (W - w_i);  at z_0 = linv (point - mean), over all used
 * j, S_0 = sum w_j K_0j, Q_0 = sum w_j^2 K_0j^2, t_0 = S_0 / W, s_0 = sqrt(Q_0) / W.  A kernel value exp(-a) with a >= 746 is +0.0 (its
 * exact value is below 0.17 * 2^-1074).  A row with w == 0 is skipped and nothing of it is
 * read into a result.
 * out (HOST, MCE_KDE_OUT doubles per system, in segment order) = {W, A2 = sum w^2, rows used, status, column, c, S_0, Q_0, M(t_0),
 * M(t_0 - s_0), M(t_0 + s_0), M_eq, reserved x 4}, M(tau) = sum over used i of w_i [t_i > tau], M_eq = sum w_i [t_i == t_0].
 * dens (optional; device, or host for _f64): n + 1 doubles, t_i (NaN for a row that is not used), t_0 last.  zout (optional, likewise):
 * the whitened rows [n][d], zeros for a row that is not used.  status 0 ok; 3 a weight that is negative or not finite; 4 a used row
 * with a value that is not finite (column: the lowest such); 5 W is not > 0; 6 fewer than 2 used rows.  With a status other than 0
 * every value is NaN; a failing system fails alone.  A system's bits depend on its own rows, d and c alone: not on its neighbours, its
 * position or the number of systems; two runs give the same bits.  Everything runs on `stream` with one host wait; five launches,
 * whatever nseg is.  Workspace: mce_kde_shift_workspace_bytes(rows of all segments, nseg, the largest d).  Argument errors (d outside
 * 1 .. 64, ld < d, negative sizes, c not positive and finite, null pointers): MCE_ERR_INVALID (no device needed); no visible device:
 * MCE_ERR_NO_DEVICE. */
#define MCE_KDE_OUT 16
#define MCE_KDE_MAX_DIM 64
typedef struct mce_kde_seg {
    const double* x;
    int64_t ld;
    int64_t n;
    int32_t d;
    const double* w;
    const double* linv;
    const double* mean;
    const double* point;
    double c;
    double* dens;
    double* zout;
} mce_kde_seg;
size_t mce_kde_shift_out_doubles(void);
size_t mce_kde_shift_workspace_bytes(int64_t nrows_total, int32_t nseg, int32_t dmax);
int mce_kde_shift_dev(const mce_kde_seg* segs, int32_t nseg, double* out, void* ws, size_t ws_bytes, void* stream);
int mce_kde_shift_f64(const mce_kde_seg* segs, int32_t nseg, double* out, int32_t device);

/* The 1-D marginal posterior densities behind marginals= (a Gaussian kernel density estimate of each of the first d parameter columns
 * on a regular grid, its mode and its highest-posterior-density regions), for MANY systems (the ready roots of a farm wave) in one
 * call.  The rule is stated in csrc/param_marginals.hpp and docs/design/marginals.md.  One system is one mce_summary_seg: x[n][ld] the
 * RAW rows and w[n] the weights of the s1 partition the estimator sums over (fs is not read); segments may differ in d and ld.  A row
 * with w == 0 is skipped and nothing of it is read into a result.  probs[np]: 1 .. MCE_MARGINALS_MAX_P probabilities in (0, 1); grid:
 * 64, 128, 256, 512 or 1024 points; scale: the factor on the normal-reference bandwidth, finite and > 0.  With W, A2, m, v, min, max as
 * mce_param_summary_dev forms them (bit for bit): ess = W W / A2, h = (scale sqrt(v)) pow(4 / (3 ess), 0.2), c = 1 / (2 h h),
 * lo = min - 3 h, step = (max + 3 h - lo) / (grid - 1), g_k = lo + k step (two roundings), rho_k = sum over used i of w_i K(c (g_k -
 * x_i)^2) / (W h sqrt(2 pi)) with K(a) = a >= 746 ? +0.0 : exp(-a).  The mode is the grid point of the largest rho (the lowest k among
 * equals).  For a probability p the grid points are ordered by rho descending, then k ascending, and rho is accumulated serially in that
 * order to Z; the region is the positions up to and including the first whose running sum is >= p Z.
 * out (HOST, packed in segment order, mce_param_marginals_out_doubles(d, np, grid) doubles per system) = {W, A2, rows used, status,
 * column, grid, np, reserved}, then the rows mean[d], var[d], sd[d], h[d], c[d], lo[d], step[d], mode[d], mode_density[d],
 * col_status[d], then per probability lower[d], upper[d], pieces[d] (the maximal runs of consecutive selected grid points), edge[d] (1
 * where the first or the last grid point is selected), then density[d][grid].  status 0 ok; 3 and 5 as mce_param_summary_dev (column
 * likewise); 6 fewer than 2 used rows: every value is NaN and that system fails alone.  col_status 0 ok; 7: sd is 0, or h, c or step
 * is not finite and > 0: that column is NaN with pieces -1, and the other columns do not notice.  A system's bits depend on its own rows,
 * probs, grid and scale alone: not on its neighbours, its position or the number of systems; two runs give the same bits; fp64, sums in
 * a fixed order, no floating-point atomics, plain stores, 64-bit row indices.  Ten launches whatever nseg is, on the caller's stream,
 * which this library synchronises once, on return.  Workspace: mce_param_marginals_workspace_bytes(rows of all segments, nseg, the
 * largest d, np, grid).  mce_param_marginals_f64 takes HOST segments, uploads them to `device` and calls the device form.  Argument
 * errors (d outside 1 .. 127, np outside 1 .. 7, a p outside (0, 1), another grid, a scale that is not finite and > 0, ld < d, negative
 * sizes, null pointers): MCE_ERR_INVALID (no device needed); no visible device: MCE_ERR_NO_DEVICE. */
#define MCE_MARGINALS_HEAD 8
#define MCE_MARGINALS_MAX_P 7
size_t mce_param_marginals_out_doubles(int32_t d, int32_t np, int32_t grid);
size_t mce_param_marginals_workspace_bytes(int64_t nrows_total, int32_t nseg, int32_t dmax, int32_t np, int32_t grid);
int mce_param_marginals_dev(const mce_summary_seg* segs, int32_t nseg, const double* probs, int32_t np, int32_t grid, double scale, double* out, void* ws,
                            size_t ws_bytes, void* stream);
int mce_param_marginals_f64(const mce_summary_seg* segs, int32_t nseg, const double* probs, int32_t np, int32_t grid, double scale, double* out, int32_t device);

/* mce_param_marginals_dev for parameters with hard prior bounds (marginals= with bounds=): the grid ends on a bound it would cross, the
 * density is Jones' linear boundary kernel in its positive form, and a grid that ends on a bound counts half a cell there in the HPD
 * sums.  The rule is stated in csrc/param_marginals_bounds.hpp and docs/design/marginals_bounds.md.  bounds: a HOST array, 2 d doubles
 * per segment in segment order, lo[d] then hi[d]; -inf / +inf: that side is open; lo < hi, neither NaN.  Everything else is taken as
 * mce_param_marginals_dev takes it.  out (HOST, mce_param_marginals_bounded_out_doubles(d, np, grid) doubles per system) = that call's
 * head with 1 in the reserved slot, then its ten per-column rows and bound_lo[d], bound_hi[d], at_lo[d], at_hi[d] (1 where the grid
 * ends on the bound), then the rows per probability and density[d][grid] as there.  col_status 8: a used value lies outside the column's
 * bounds; that column is NaN with pieces -1, and the other columns do not notice.  A column whose two sides are open has the bits
 * mce_param_marginals_dev gives it.  A system's bits depend on its own rows, bounds, probs, grid and scale alone.  Ten launches whatever
 * nseg is, on the caller's stream, which this library synchronises once, on return.  Workspace:
 * mce_param_marginals_bounded_workspace_bytes(rows of all segments, nseg, the largest d, np, grid).  mce_param_marginals_bounded_f64
 * takes HOST segments.  Argument errors (those of mce_param_marginals_dev, a null bounds, a pair of bounds that is not lo < hi):
 * MCE_ERR_INVALID (no device needed). */
size_t mce_param_marginals_bounded_out_doubles(int32_t d, int32_t np, int32_t grid);
size_t mce_param_marginals_bounded_workspace_bytes(int64_t nrows_total, int32_t nseg, int32_t dmax, int32_t np, int32_t grid);
int mce_param_marginals_bounded_dev(const mce_summary_seg* segs, int32_t nseg, const double* bounds, const double* probs, int32_t np, int32_t grid, double scale,
                                    double* out, void* ws, size_t ws_bytes, void* stream);
int mce_param_marginals_bounded_f64(const mce_summary_seg* segs, int32_t nseg, const double* bounds, const double* probs, int32_t np, int32_t grid, double scale,
                                    double* out, int32_t device);

/* The 2-D joint posterior densities behind contours= (a product-Gaussian kernel density estimate of every pair of chosen parameter
 * columns on a regular grid x grid, its mode and its credible regions), for MANY systems in one call.  The rule is stated in
 * csrc/param_contours.hpp and docs/design/contours.md.  One system is one mce_summary_seg as for mce_param_marginals_dev.  cols[nc]: a
 * strictly increasing list of 2 .. MCE_CONTOURS_MAX_COLS columns, every one below every segment's d; the pairs are (cols[s], cols[t]),
 * s < t, in the order (0,1), (0,2), .., (nc-2, nc-1), P = nc (nc - 1) / 2 of them, the first column of a pair its x axis.  probs[np]:
 * 1 .. MCE_MARGINALS_MAX_P probabilities in (0, 1); grid: 32 or 64; scale: finite and > 0.  With the moments as mce_param_summary_dev
 * forms them (bit for bit): h = (scale sqrt(v)) pow(1 / ess, 1 / 6), c = 1 / (2 h h), lo = min - 3 h, step = (max + 3 h - lo) /
 * (grid - 1), E_j[r][k] = K(c_j (g_jk - x_rj)^2) with K(a) = a >= 746 ? +0.0 : exp(-a), rho[kx][ky] = sum over used r of (w_r E_i[r][kx])
 * E_j[r][ky] / (W h_i h_j 2 pi).  The mode is the cell of the largest rho (the lowest kx * grid + ky among equals).  For a probability p
 * the cells are ordered by rho descending, then flat index ascending, and rho is accumulated serially in that order to Z; the region is
 * the positions up to and including the first whose running sum is >= p Z.
 * out (HOST, packed in segment order, mce_param_contours_out_doubles(nc, np, grid) doubles per system) = {W, A2, rows used, status,
 * column, grid, np, nc}, then the rows col[nc], mean, var, sd, h, c, lo, step, col_status, then mode_x[P], mode_y, mode_density,
 * pair_status, then per probability level[P] (the contour height), cells, lower_x, upper_x, lower_y, upper_y (the bounding box in grid
 * points), edge (1 where a selected cell lies on the grid's border), then density[P][grid][grid], kx the slow index.  status 0 ok; 3, 5
 * and 6 as mce_param_marginals_dev: every value is NaN and that system fails alone.  col_status 7 as there, on this rule's h, c and
 * step; a pair with such a column has pair_status 7, NaN values and cells -1, and the other pairs do not notice.  A pair's bits depend
 * on its system's rows, its two columns, grid and scale alone; two runs give the same bits; fp64, sums in a fixed order, no
 * floating-point atomics, plain stores, 64-bit row indices.  Ten launches whatever nseg is, on the caller's stream, which this library
 * synchronises once, on return.  Workspace: mce_param_contours_workspace_bytes(rows of all segments, nseg, the largest d, nc, np, grid).
 * mce_param_contours_f64 takes HOST segments, uploads them to `device` and calls the device form.  Argument errors: MCE_ERR_INVALID (no
 * device needed); no visible device: MCE_ERR_NO_DEVICE. */
#define MCE_CONTOURS_HEAD 8
#define MCE_CONTOURS_MAX_COLS 32
size_t mce_param_contours_out_doubles(int32_t nc, int32_t np, int32_t grid);
size_t mce_param_contours_workspace_bytes(int64_t nrows_total, int32_t nseg, int32_t dmax, int32_t nc, int32_t np, int32_t grid);
int mce_param_contours_dev(const mce_summary_seg* segs, int32_t nseg, const int32_t* cols, int32_t nc, const double* probs, int32_t np, int32_t grid, double scale,
                           double* out, void* ws, size_t ws_bytes, void* stream);
int mce_param_contours_f64(const mce_summary_seg* segs, int32_t nseg, const int32_t* cols, int32_t nc, const double* probs, int32_t np, int32_t grid, double scale,
                           double* out, int32_t device);

/* The same for chains sampled under hard prior bounds (csrc/param_contours.hpp's steps 3" .. 8"; docs/design/contours_bounds.md).
 * bounds: a HOST array of 2 nc doubles per segment, lo[nc] then hi[nc] of the chosen columns, -inf / +inf where a side is open; a pair
 * that is not lo < hi, or a null pointer: MCE_ERR_INVALID before any device call.  A grid ends on a bound it would cross (at_lo /
 * at_hi), the density is the three-term linear boundary kernel of the product kernel on the rectangle in its positive form -- next to S
 * the first-moment sums R_x and R_y are formed for every column that is not open, and f0 exp(min(f1 / f0, 4) - 1) is reported -- and
 * the running sum of a region gives a cell on a grid end that lies on a bound half its weight per such axis.  A used value outside its
 * bounds: col_status 8 (7 comes first); a pair takes the status of its failing column, the x axis' first.  A pair whose two columns are
 * open has mce_param_contours_dev's bits.  out: mce_param_contours_bounded_out_doubles(nc, np, grid) doubles per system: as above with
 * the column rows bound_lo[nc], bound_hi, at_lo, at_hi after col_status.  The same ten launches and one wait. */
size_t mce_param_contours_bounded_out_doubles(int32_t nc, int32_t np, int32_t grid);
size_t mce_param_contours_bounded_workspace_bytes(int64_t nrows_total, int32_t nseg, int32_t dmax, int32_t nc, int32_t np, int32_t grid);
int mce_param_contours_bounded_dev(const mce_summary_seg* segs, int32_t nseg, const int32_t* cols, int32_t nc, const double* bounds, const double* probs, int32_t np,
                                   int32_t grid, double scale, double* out, void* ws, size_t ws_bytes, void* stream);
int mce_param_contours_bounded_f64(const mce_summary_seg* segs, int32_t nseg, const int32_t* cols, int32_t nc, const double* bounds, const double* probs, int32_t np,
                                   int32_t grid, double scale, double* out, int32_t device);

/* The farm: MANY chain files -> fp64 on the device in one pass per wave (the reference's Planck grid, planck_mcevidence.py:306-348:
 * thousands of small roots).  A farm reader handle is created once per device and reused for every wave: it owns one stream, device
 * scratch and ONE pinned staging buffer of `capacity_bytes` (a multiple of 4096); no allocation and no stream per file or per wave (an
 * array a wave does not fit is grown once and counted in the stats).  A handle belongs to one thread.
 * Layout of a wave: the caller writes file f's bytes into the staging buffer at file_off[f] -- a multiple of 4096, file_off[0] = 0 --
 * with at least one byte behind every file: file_off[f + 1] >= file_off[f] + file_len[f] + 1, rounded up to 4096; wave_bytes (a
 * multiple of 4096, <= capacity) ends the last file in the same way.  The library fills every gap with '\n' on the device, so a file
 * boundary behaves like the end of a file.  TWO STEPS, as mce_chain_dev_open / _read_dev:
 *   structure  uploads the wave (one copy) and finds, per file, its tokens, rows and columns: files[f] = {tok_base, ntok, nrows, ncols,
 *              status}; *ntok_total = the tokens of the wave.  A ragged file (the rule of mce_chain_dev_open inside the file's tokens)
 *              has status MCE_FARM_RAGGED and fails ALONE; a file with no token has 0 rows and 0 columns.
 *   parse      the caller allocates d_out[ntok_total] on the handle's device in between; global token k is written to d_out[k], so file
 *              f's array [nrows, ncols] starts at d_out + files[f].tok_base.  Undecided tokens are converted by the host's strtod from the
 *              staging bytes (which must stay untouched until parse returns) and go up in one copy; a field that is not a number sets its
 *              file's status to MCE_FARM_NOT_A_NUMBER and bad_row / bad_col (0-based row, 1-based column inside the file); the other
 *              files are unaffected.  The handle's stream is synchronised on return of either step.
 *   stats[12]  {waves, files, device allocations since creation, ... in the last wave, arrays grown, tokens of the last wave, tokens
 *              patched, ms upload, ms structure, ms parse, ms patch, capacity}
 * Argument errors: MCE_ERR_INVALID (no device needed); no visible device: MCE_ERR_NO_DEVICE. */
#define MCE_FARM_OK 0
#define MCE_FARM_RAGGED 1
#define MCE_FARM_NOT_A_NUMBER 2
typedef struct mce_farm_file {
    int64_t tok_base, ntok, nrows, ncols, status, bad_row, bad_col;
} mce_farm_file;
int mce_chain_farm_create(int64_t capacity_bytes, int32_t device, void** handle, void** staging);
void mce_chain_farm_destroy(void* handle);
int mce_chain_farm_structure(void* handle, const int64_t* file_off, const int64_t* file_len, int32_t nfiles, int64_t wave_bytes,
                             mce_farm_file* files, int64_t* ntok_total);
int mce_chain_farm_parse(void* handle, double* d_out, mce_farm_file* files, int32_t nfiles);
int mce_chain_farm_stats(void* handle, double* stats, int32_t nstats);
/* mce_chain_gather_dev (parameters, weight, likelihood) and mce_chain_reduce_dev for EVERY unthinned root of a wave in one set of
 * launches.  Root r owns the next root_nparts[r] entries of `parts` (its files after burn-in, as for mce_chain_gather_dev; empty parts
 * allowed, a root needs one row) and has root_ncols[r] columns.  Outputs, roots one after the other: d_params (rows * (ncols - itheta)
 * doubles per root), d_w / d_like / d_fs (one per row), out[4 * r ..] (host) = mce_chain_reduce_dev's out of root r.  The reductions
 * run in the root's own row numbering, in mce_chain_reduce_dev's order: a root's bits do not depend on its neighbours.  Synchronises
 * the stream. */
size_t mce_chain_farm_prep_workspace_bytes(int32_t nroots, int32_t nparts, int64_t nrows);
int mce_chain_farm_prep_dev(const int32_t* root_nparts, const int64_t* root_ncols, int32_t nroots, const mce_chain_part* parts, int32_t nparts,
                            int32_t iw, int32_t ilike, int32_t itheta, int32_t pos_lnp, double* d_params, double* d_w, double* d_like,
                            double* d_fs, double* out, void* ws, size_t ws_bytes, void* stream);

/* Spatial pruning of the fp16-filter search for low-dimensional, large reference sets (d <= 13):
 * both point sets are put in k-d order on the device (cells of 32 rows) and every wave of 64 queries
 * visits the reference chunks nearest-box-first, multiplies only the 32-row tiles whose box is within
 * reach, and stops once no remaining chunk can hold a neighbour.  Same neighbours, distances and
 * tie-breaks as the exhaustive search.  0 (default): used where it was measured faster -- d <= 4 from
 * 100 k reference rows, d = 5 from 125 k, d = 6 from 150 k, d = 7 from 250 k, d = 8 from 500 k (the table is capi_common.hpp: kPruneAutoMinRows),
 * and at least 32 k queries, no fewer than an eighth of the reference rows; 1: never; 2: whenever the shape allows it
 * (d <= 15, K <= 16).  Process-wide default (per call: mce_options). */
int mce_set_prune_mode(int mode);
int mce_get_prune_mode(void);

/* Symmetric sweep of an auto-evidence search (X and Y are ONE buffer, nq == nr: reference
 * MCEvidence.py:1100-1104, `nbrs.fit(samples); nbrs.kneighbors(samples)`).  d(i,j) = d(j,i), so every
 * 32x32 tile of the exhaustive fp16 filter sweep is needed by both of its sides; here it is multiplied once:
 * the rows are sorted by distance from the mean, a prepass bounds every row's K-th distance, every block of
 * 512 rows sweeps only the blocks before it, and each tile is gated for the streamed rows
 * too; their candidates are merged into the lists afterwards.  Same neighbours, distances and tie-breaks as
 * the exhaustive search.  0 (default): where it was measured faster and pruning does not apply -- from 768 blocks of
 * 512 rows (393 k rows; twice that with K > 12) where the filter takes one 16-wide k-step (d <= 15: capi.hip
 * f16_ksteps(d) = (d + 16) / 16), from 257 blocks (131 k rows) with two (d <= 31), from 193 (99 k rows) beyond (kSymAutoMinBlocks);
 * 1: never; 2: whenever the shape allows it (fp16-filter shapes with K <= 16, more than 512 rows).
 * Process-wide default (per call: mce_options); the environment variable MCE_SYM sets the initial value.
 * Multi-GPU: up to four ranks mce_knn_dotp_part_f64 partitions such a search by ranges of the sorted blocks (symmetric
 * within a rank's range, column side only against the other ranks' rows) -- no exchange between the ranks; larger jobs
 * shard the query rows. */
int mce_set_sym_mode(int mode);
int mce_get_sym_mode(void);
/* Work actually done by the last pruned search launched by this thread through a *_dev entry point
 * (its workspace must still be alive): fraction of (query block, reference chunk) pairs staged, and
 * fraction of (wave, 32-row tile) products multiplied.  Synchronises the device. */
int mce_last_prune_stats(double *chunk_fraction, double *tile_fraction);

/* Measurement hook: while enabled, the search-kernel launch of every call on this thread
 * is bracketed by hipEvents recorded on the launch stream (no synchronisation);
 * mce_last_kernel_ms() waits for the brackets recorded since the last enable and returns
 * the MEAN search-kernel time per call in ms (-1 if none; a call that searches two query ranges --
 * DESIGN.md 3.0, trailing round -- counts once, with both launches).  Used by bench.py for the
 * roofline figure. */
void mce_set_profiling(int on);
double mce_last_kernel_ms(void);
/* What the last search on this thread asked of the matrix cores, for rooflines that follow from a profile (bench.py):
 *   out[0]  MFMA flops EXECUTED by the dominant kernel (the one mce_last_kernel_ms() brackets) -- a symmetric sweep
 *           multiplies each pair of rows once, so this is about half of the all-pairs figure; -1: only device counters
 *           know (pruned walk: mce_last_prune_stats)
 *   out[1]  the same over every launch of the search (prepass / seed phases included)
 *   out[2]  milliseconds of the whole search, packing to the last list kernel (HIP events on the launch stream, mean per
 *           search since mce_set_profiling(1)); -1 without profiling
 *   out[3]  mce_last_kernel_ms()
 * Bookkeeping of the measurement hooks; no counterpart in the reference. */
int mce_last_search_stats(double* out, int32_t n);

/* Test hook: one 32 x 32 tile of the filter's matrix product exactly as the search kernels issue it
 * (v_mfma_f32_32x32x16_f16, `kst` chained k-steps): out[row * 32 + query] = sum_k yprime[row][k] * xprime[query][k], rows of
 * 16 * kst fp16 values (bit patterns) each.  tests/test_gpu_parity.py::test_mfma_error_model checks the error model the
 * rigorous filter bound assumes (knn_f16.hpp) against it.  No counterpart in the reference. */
int mce_debug_mfma_tile_f16(const uint16_t* yprime, const uint16_t* xprime, int32_t kst, float* out, int32_t device);
/* the same for `ntiles` independent tiles in one launch (yprime, xprime: [ntiles][32][16 kst]; out: [ntiles][32][32]) */
int mce_debug_mfma_tiles_f16(const uint16_t* yprime, const uint16_t* xprime, int32_t kst, int32_t ntiles, float* out, int32_t device);

#ifdef __cplusplus
}
#endif
#endif /* MCEVIDENCE_HIP_H */
