/* gpzoo_hip.h -- C ABI of libgpzoo_hip.so (MI355X / gfx950).
 *
 * The reference (luisdiaz1997/GPzoo) is pure Python/torch and has no FFI of its
 * own; this ABI is what a maintainer binds (ctypes stub in INTEGRATION.md) to
 * replace the torch ops on the SVGP/NSF hot path.  Each entry point cites the
 * reference lines whose arithmetic it replaces (paths under /root/reference).
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is DEVICE memory owned by the
 *    caller unless marked "host"; the library never allocates user-visible
 *    memory; scratch comes from a caller workspace sized by *_workspace_bytes.
 *  - the workspace need not be cleared by the caller and may hold anything (every entry writes, or clears, each part
 *    of it before reading it); outputs are fully written on success except where stated: the opaque buffers
 *    wt_cache (the unused columns of a short last chunk's slot stay untouched), factor_cache and the VNNGP state
 *    (blocks above the diagonal of the inverse factor are neither stored nor loaded) -- DESIGN.md, "Scratch and
 *    output initialisation".
 *  - all launches are asynchronous on `stream` (a hipStream_t passed as void*).
 *  - return 0 on success, negative on bad arguments / launch errors
 *    (gpz_last_error() holds the message, per thread).
 *  - dtype: GPZ_F32 = 0, GPZ_F64 = 1.  Matrices are row-major, batched over a
 *    leading latent axis L with an explicit batch stride (in elements).
 *  - non-PD input to a factorisation: LAPACK-style info[b] = k > 0 written to
 *    device memory (order of the first non-positive leading minor); the Python
 *    wrapper turns it into torch.linalg.LinAlgError like gp.py:213/270/360.
 *
 * Additions under version 212 (the version number is unchanged; nothing existing moved): gpz_spatial_knn,
 * gpz_morans_i and their *_workspace_bytes queries -- the spatial statistics of dims_autocorr (utilities.py:131-156);
 * gpz_nmf_kl_update, gpz_nmf_kl_divergence and gpz_nmf_kl_workspace_bytes -- the KL multiplicative-update NMF behind
 * regularized_nmf (utilities.py:253-299, sklearn's NMF(solver='mu', beta_loss='kullback-leibler'));
 * GPZ_KERNEL_MATERN12 and GPZ_KERNEL_MATERN52 -- two more values of gpz_kernel_desc.kind, accepted wherever
 * GPZ_KERNEL_MATERN32 is (gpz_kfill, gpz_kgrad, gpz_svgp_forward / _backward and the Poisson entries);
 * gpz_vnngp_forward / _backward (and their workspace queries) accept GPZ_KERNEL_MATERN32, _MATERN12 and _MATERN52 next to
 * GPZ_KERNEL_RBF -- the set of accepted kind values grew, nothing else about the entries changed;
 * gpz_knn_mean and gpz_knn_mean_workspace_bytes -- the exact K-nearest mean of the factors at the inducing points behind
 * smooth_spatial_factors (utilities.py:50-68, sklearn's KNeighborsRegressor.predict);
 * gpz_kmeans_seed, gpz_kmeans_lloyd, gpz_kmeans_assign and their *_workspace_bytes queries -- k-means++ seeding and Lloyd's
 * iterations behind kmeans_inducing_points (the notebooks' sklearn KMeans(n_clusters=M).fit(X).cluster_centers_ for Z);
 * gpz_kernel_gram, gpz_kernel_gram_workspace_bytes and gpz_kernel_gram_plan -- the normal equations K_zx K_xz + jitter I and
 * K_zx F^T of the kernel least-squares start for gp.mu behind project_factors_to_inducing (the notebooks' hand-written
 * Kzx @ Kxz / cholesky_solve composition), in one pass over X without a stored K_zx;
 * gpz_poisson_nsf_sparse, gpz_poisson_nsf_sparse_workspace_bytes and gpz_poisson_nsf_sparse_plan -- gpz_poisson_nsf for
 * counts stored as their non-zeros: the same outputs as exact sums over the non-zeros;
 * gpz_nmf_kl_sparse_update, gpz_nmf_kl_sparse_divergence, gpz_nmf_kl_sparse_workspace_bytes and gpz_nmf_kl_sparse_plan --
 * gpz_nmf_kl_update / _divergence over the same stored non-zeros, and gpz_counts_matmul with its workspace query -- the
 * products of those counts with a thin dense matrix that the NNDSVD start of that factorisation needs;
 * gpz_poisson_deviance and gpz_poisson_deviance_sparse, each with its *_workspace_bytes and host-only *_plan query -- the
 * Poisson deviance of counts (dense, or stored as their non-zeros) under the predictive mean rate of a fitted factor model,
 * per gene, per spot and in total, with the null model's deviance: the score of held-out spots, which the reference's
 * anndata_to_train_val prepares (Dval) and nothing in it computes;
 * gpz_nb_nsf, gpz_nb_nsf_workspace_bytes and the host-only gpz_nb_nsf_plan -- the training step of gpz_poisson_nsf under a
 * negative-binomial likelihood with one inverse dispersion per gene (the nsf paper's lik="nb");
 * gpz_nb_nsf_sparse, gpz_nb_nsf_sparse_workspace_bytes and the host-only gpz_nb_nsf_sparse_plan -- gpz_nb_nsf for counts
 * stored as their non-zeros: a dense pass over the batch that reads no counts plus sums over the non-zeros;
 * gpz_nb_deviance and gpz_nb_deviance_sparse, each with its *_workspace_bytes and host-only *_plan query -- the NB deviance,
 * the NB log density and the Poisson log density of held-out counts under the predictive mean rate and a per-gene theta;
 * gpz_gaussian_fa and the host-only gpz_gaussian_fa_plan -- the exact expected Gaussian log-likelihood of the real-valued
 * factor models (RSF over a GP prior, FA over an i.i.d. one) and its gradients; its scratch is the explicit argument
 * `partials`, sized by the plan query;
 * gpz_gaussian_fa_sparse and the host-only gpz_gaussian_fa_sparse_plan -- gpz_gaussian_fa for expression stored as its
 * non-zeros minus a per-gene offset (centred log-normalised counts): the same outputs as exact sums over the non-zeros
 * plus Lt x Lt Gram matrices; its scratch is `partials` again, sized by the plan query's workspace_bytes;
 * gpz_gene_deviance_sparse and gpz_gene_morans_i_sparse, each with its host-only *_plan query -- two per-gene scores of
 * counts stored as their non-zeros, for ranking and selecting genes ahead of a fit: the Poisson / binomial deviance against a
 * constant-rate null (scry's devianceFeatureSelection) and Moran's I over the spots' K-neighbour graph (squidpy's
 * spatial_autocorr, one gene per column); their scratch is `partials`, sized by the plan query's partials_bytes;
 * gpz_gene_dispersion_sparse and the host-only gpz_gene_dispersion_sparse_plan -- the maximum-likelihood negative-binomial
 * inverse dispersion of every gene of the same stored counts under the constant-rate null, with its gain over Poisson: which
 * genes are overdispersed, and where theta starts (edgeR / DESeq2 / glmGamPoi's gene-wise estimate); scratch `partials` again;
 * gpz_count_residuals, gpz_count_residuals_sparse, gpz_residual_morans_i, gpz_residual_morans_i_sparse and the host-only
 * gpz_residual_morans_i_plan -- Pearson or deviance residuals of counts under the predictive mean rate of a fitted count
 * model, and Moran's I of every gene's residuals over the spots' K-neighbour graph (is spatial structure left in what the
 * model did not explain, and in which genes), dense counts or counts stored as their non-zeros; scratch `partials` again;
 * gpz_gene_morans_perm_sparse, gpz_morans_perm_rows and their host-only *_plan queries -- Moran's I of every gene under P
 * relabellings of the spots (the permutation null of squidpy's spatial_autocorr(n_perms=)): the simulated values, the counts
 * behind the pseudo p-value and the simulated mean and variance, from stored non-zeros or dense rows; scratch `partials`;
 * gpz_gene_spatial_stats_sparse, gpz_spatial_stats, gpz_gene_autocorr_perm_sparse, gpz_autocorr_perm_rows and their host-only
 * *_plan queries -- Moran's I and Geary's C (squidpy's spatial_autocorr(mode="geary")) of every gene with its mean, variance and
 * kurtosis, which the randomisation variances of both statistics need, and the permutation entries with the statistic as an
 * argument; scratch `partials`;
 * gpz_residual_spatial_stats, gpz_residual_spatial_stats_sparse, gpz_residual_autocorr_perm, gpz_residual_autocorr_perm_sparse
 * and the host-only gpz_residual_autocorr_perm_plan -- Geary's C and the kurtosis beside Moran's I of every gene's residuals,
 * and either statistic under P relabellings of the spots while the residual slab is resident (the permutation null after
 * the fit); scratch `partials`;
 * gpz_gaussian_residuals, gpz_gaussian_residual_stats, gpz_gaussian_residual_perm, their *_sparse forms and the host-only
 * gpz_gaussian_residual_plan -- the same residual diagnostics for the Gaussian factor models (RSF, FA): Pearson, response or
 * predictive residuals of real-valued expression, dense or stored as its non-zeros minus a per-gene offset; scratch `partials`;
 * gpz_gene_kernel_project_sparse, gpz_gene_gp_profile and their host-only *_plan queries -- the two device steps of the sparse-GP
 * test for spatially variable genes (SpatialDE / nnSVG's question, scored by Titsias' collapsed bound): K_zx Y^T of every gene
 * over its stored entries for a grid of length scales with K_zx generated and never stored, and the per-gene maximum of the
 * bound over the noise-to-signal ratio; scratch `partials` for the first, none for the second.
 */
#ifndef GPZOO_HIP_H
#define GPZOO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPZ_VERSION 212

enum { GPZ_F32 = 0, GPZ_F64 = 1 };

/* covariance families: every kernel class of gpzoo/kernels.py maps to one */
enum {
  GPZ_KERNEL_RBF = 0,      /* RBF, NSF_RBF, batched_RBF      kernels.py:34-59,106-155  */
  GPZ_KERNEL_MATERN32 = 1, /* batched_Matern32               kernels.py:6-30           */
  GPZ_KERNEL_MGGP_RBF = 2, /* MGGP_RBF, MGGP_NSF_RBF, batched_MGGP_RBF  kernels.py:62-104,158-228 */
  GPZ_KERNEL_DISTANCE = 3, /* plain Euclidean distance (return_distance=True, kernels.py:118,125-126) */
  GPZ_KERNEL_MATERN12 = 4, /* batched_Matern12: sigma^2 exp(-r / l), the closed form of a batched_Matern32 subclass
                              whose covariance() is the exponential (Ornstein-Uhlenbeck) kernel  kernels.py:6-30 */
  GPZ_KERNEL_MATERN52 = 5  /* batched_Matern52: sigma^2 (1 + v + v^2 / 3) exp(-v), v = sqrt(5) r / l  (same) */
};

/* Hyper-parameters of one covariance family for L independent latents.
 * sigma / lengthscale / group_a: device arrays of L values of dtype `dtype`.
 * group_a is the EFFECTIVE multiplier of the squared group distance
 * (a, a^2 or |a| depending on the class: kernels.py:187 / :222 / :87), NULL
 * unless kind == GPZ_KERNEL_MGGP_RBF.  group_r2 is the (G,G) table of squared
 * distances between group embeddings (dtype `dtype`); group_pow = p/2, the
 * exponent of the denominator (kernels.py:189, :224, :89). */
typedef struct gpz_kernel_desc {
  int32_t kind;
  int32_t n_latent;
  int32_t dtype;
  int32_t n_groups;
  const void* sigma;
  const void* lengthscale;
  const void* group_a;
  const void* group_r2;
  double group_pow;
} gpz_kernel_desc;

int gpz_version(void);
const char* gpz_last_error(void);
/* sha256 (32 hex digits) of the source files this binary was built from ("unknown" for a hand-made build): the Python
 * loader refuses a library whose value differs from the sources lying next to it (a stale binary). */
const char* gpz_source_hash(void);

/* K[l][i][j] = k_l(A_i, B_j) (+ jitter where i == j if jitter != 0).
 * Replaces kernel.forward(X, Z) -- kernels.py:29-30, 57-58, 98-104, 118-130,
 * 146-155, 176-191, 211-228 -- and add_jitter (utilities.py:407-418) fused.
 * A (nA,d), B (nB,d) of k->dtype; gA/gB int64 group ids (MGGP only, else NULL).  An id outside
 * [0, n_groups) -- IndexError in the reference (kernels.py:99-100, 177-178, 209-210) -- is read as group 0
 * here (no out-of-bounds access); gpz_svgp_forward reports it through info (see there).
 * K has dtype out_dtype, row stride ldk, latent stride stride_k (elements).
 * Distances are evaluated by direct differencing in the output precision. */
int gpz_kfill(const gpz_kernel_desc* k, const void* A, int64_t nA, const void* B, int64_t nB,
              int32_t d, const int64_t* gA, const int64_t* gB, void* K, int64_t ldk,
              int64_t stride_k, double jitter, int32_t out_dtype, void* stream);

/* Backward of gpz_kfill: contracts Kbar = dLoss/dK (L,nA,nB; dtype k->dtype, row stride ldk, latent stride
 * stride_k) with dK/d(sigma, lengthscale, group_a) and dK/dA -- what torch autograd sends through
 * kernel.forward in the reference, where kernels are ordinary traced modules (kernels.py:14-30, 42-58,
 * 75-104, 114-130, 139-155, 176-228; e.g. the inline ExactGP of exact_mggp.ipynb).  Outputs fp64:
 * grad_theta (L,4) = d/dsigma, d/dlengthscale, d/dgroup_a (effective multiplier), 0;  grad_A (nA,4), first d
 * columns used, summed over latents (NULL: skipped).  For dLoss/dB call it again with A and B (and the groups)
 * swapped and Kbar transposed.  Matern-3/2 and -5/2: dK/dA at coincident points is 0 (its limit; the reference's
 * autograd yields NaN there); Matern-1/2 has a kink there and 0 is returned as well.  GPZ_KERNEL_DISTANCE is not differentiable here. */
size_t gpz_kgrad_workspace_bytes(int64_t nA, int32_t n_latent);
int gpz_kgrad(const gpz_kernel_desc* k, const void* A, int64_t nA, const void* B, int64_t nB, int32_t d,
              const int64_t* gA, const int64_t* gB, const void* Kbar, int64_t ldk, int64_t stride_k,
              double* grad_theta, double* grad_A, void* ws, size_t ws_bytes, void* stream);

/* In-place lower Cholesky of `batch` (M,M) matrices stored as `dtype` (the arithmetic is fp64 either way:
 * "factor precision"), zeros written above the diagonal; info[b] as described above.  Replaces
 * torch.linalg.cholesky at gp.py:213, 270, 360.  Default: ONE launch, a left-looking dataflow over 128 x 128 tiles
 * (csrc/coop.hip: diagonal blocks factored in LDS, every tile's sum kept in its owner's registers on
 * v_mfma_f64_16x16x4_f64, hand-offs through flags).  Orders beyond that launch's task list, or
 * GPZ_FACTOR_PATH=launches, take the blocked right-looking chain of launches (csrc/factor.hip: LDS-resident diagonal
 * panel, MFMA panel solve and trailing SYRK/GEMM update).  info[b] = -7 anywhere (a hand-off of the one-launch path
 * timed out) invalidates the WHOLE batch: matrices the aborting workgroups had not reached are left unfactored. */
/* Which factorisation matrices of order M take: 1 = the one-launch tile dataflow (Cholesky and, with_inverse, the
 * triangular inverse in the same launch; csrc/coop.hip), 0 = one launch per step of the blocked algorithm (orders whose
 * task list exceeds the kernel-argument space, or GPZ_FACTOR_PATH=launches in the environment). */
int gpz_factor_path(int64_t M, int32_t with_inverse);
size_t gpz_potrf_workspace_bytes(int64_t M, int64_t batch);
int gpz_potrf_batched(void* A, int32_t dtype, int64_t M, int64_t lda, int64_t stride_a, int64_t batch,
                      int32_t* info, void* ws, size_t ws_bytes, void* stream);

/* X = Lc^{-1} B for `batch` lower-triangular (M,M) factors and (M,N) right-hand sides stored as `dtype`
 * (fp64 arithmetic), X written over B.  Replaces torch.linalg.solve_triangular at gp.py:276 (and each half
 * of cholesky_solve at gp.py:218, 365).  Blocked forward substitution: the 128x128 diagonal blocks are
 * inverted in LDS, then one MFMA GEMM per block row applies X_k = D_k (B_k - sum_{j<k} L_kj X_j) in place.
 * (gpz_svgp_forward does not call this: it forms the explicit inverse once per evaluation and applies it to
 * every N-chunk as one triangular product.) */
size_t gpz_trsm_workspace_bytes(int64_t M, int64_t N, int64_t batch);
int gpz_trsm_lln_batched(const void* Lc, int64_t ldl, int64_t stride_l, void* B, int64_t ldb,
                         int64_t stride_b, int32_t dtype, int64_t M, int64_t N, int64_t batch, void* ws,
                         size_t ws_bytes, void* stream);

/* One evaluation of the SVGP / WSVGP forward pass and (optionally) the
 * closed-form Gaussian ELBO, batched over L latents and tiled over N:
 *   Kzz(+jitter) -> Cholesky -> L^{-1} -> per N-chunk { Kzx fill, Wt = L^{-1} Kzx,
 *   Lu^T Wt, column reductions } -> q(F) mean / scale, KL per latent, ELBO.
 * Replaces WSVGP.forward gp.py:260-306, SVGP.forward gp.py:183-232 (+
 * svgp_forward utilities.py:382-397), MGGP_* gp.py:341-399, whitened_KL
 * utilities.py:27-36, kl_divergence(qU,pU) at utilities.py:481, and the ELBO
 * assembly of mggp_test_exact.ipynb:157-159.
 * dtype = storage/GEMM type of X, Z, mu, Lu_raw, y, mean, scale (k.dtype must
 * match).  Kzz, its Cholesky factor and inverse are carried in fp64 in both modes.
 */
/* gpz_svgp_problem.flags: which kernels the forward pass takes for its two big fp32 products (results agree bit for
 * bit in Wt on every path; 0 = the library's choice: the fill + wide-tile products for M > 512, the panel kernel for
 * M <= 512 where it is the faster one -- see GPZ_SVGP_PANEL_PRODUCTS) */
#define GPZ_SVGP_MATERIALIZE_KZX 1  /* write every Kzx chunk to HBM with the stand-alone fill and run the triangular
                                     * product on it -- the reference's structure, gp.py:255 + :276 */
#define GPZ_SVGP_NARROW_TILES 2     /* the 128 x 128-tile kernel every other precision uses (csrc/gemm.hip) instead of
                                     * the wide-tile one (csrc/gemmw.hip); implies a materialised Kzx */
#define GPZ_SVGP_GENERATE_KZX 4     /* fp32 RBF / Matern-3/2, d <= 2: stage 1 generates its covariance operand inside the
                                     * product (csrc/gemmw.hip) and Kzx is never written */
#define GPZ_SVGP_PANEL_PRODUCTS 8   /* fp32, M <= 512: both products panel by panel in ONE launch (csrc/gemmp.hip): a workgroup
                                     * holds 64 columns x all rows in LDS from the covariance to the column statistics.
                                     * RBF / Matern-3/2 on <= 2-D inputs: the panel is computed inside the kernel and Kzx
                                     * never exists; other kernel families: it is read from the stand-alone fill's Kzx.
                                     * Wt reaches memory only when retained.  Same Wt bits; mean / scale differ from the
                                     * tile path by fp32 rounding (other summation order of the statistics).  The
                                     * library's own choice (flags == 0) in the first case for every M <= 512 and in the
                                     * second for 128 < M <= 512; with this flag wherever it applies; ignored elsewhere
                                     * and next to any of the three flags above. */
/* gpz_svgp_backward only: which form the N-sized work of the pass takes (0 = the library's choice by N / M; the
 * gradients agree to rounding).  ALGEBRA: one weighted symmetric accumulation H += W diag(gv2) W^T per chunk (and, with
 * grad_theta / grad_Z, one dense product for Kbar_x) plus M x M products; CLASSIC: the products autograd would run --
 * Pbar, W Pbar^T (and Wbar, Kbar_x, Kbar_x W^T). */
#define GPZ_SVGP_BACKWARD_ALGEBRA 16
#define GPZ_SVGP_BACKWARD_CLASSIC 32

typedef struct gpz_svgp_problem {
  gpz_kernel_desc k;
  int32_t dtype;
  int32_t whitened;      /* 1: WSVGP (gp.py:260), 0: SVGP (gp.py:183) */
  int32_t d;             /* input dimension */
  int32_t flags;         /* GPZ_SVGP_* bits; 0 = defaults */
  int64_t N, M;
  const void* X;         /* (N,d) */
  const void* Z;         /* (M,d) */
  const int64_t* gX;     /* (N,) MGGP only */
  const int64_t* gZ;     /* (M,) MGGP only */
  const void* mu;        /* (L,M) */
  const void* Lu_raw;    /* (L,M,M) unconstrained: diag is exponentiated */
  double jitter;
  double var_clamp_min;  /* un-whitened only: clamp(cov, min) gp.py:228 (1e-6) / :378 (5e-2) */
  const void* y;         /* (L,N) targets or NULL: no likelihood terms */
  double noise_sd;       /* softplus(noise) of likelihoods.py:33 */
  /* outputs (any may be NULL) */
  void* mean;            /* (L,N) dtype */
  void* scale;           /* (L,N) dtype: sqrt of the predictive variance */
  void* Lu;              /* (L,M,M) dtype: constrained scale_tril of q(U) */
  void* chol;            /* (L,M,M) dtype: Cholesky factor of Kzz + jitter I */
  double* kl;            /* (L,) */
  double* loglik;        /* (L,) sum_n log N(y; mean, s^2) - var / (2 s^2) */
  double* elbo;          /* (1,) sum_l loglik - kl */
  int32_t* info;         /* (L,) potrf info; info[0] = -1: a group id in gX / gZ is outside [0, n_groups)
                          * (LAPACK's "illegal argument"; the Python wrapper raises IndexError like the reference) */
  /* optional cache of everything that depends only on (Z, kernel hyper-parameters, jitter):
   * chol(Kzz), its inverse and sum(log diag).  NULL: recompute every call like the reference
   * (SURVEY §3.3).  Non-NULL (gpz_svgp_factor_cache_bytes bytes, caller owned): filled when
   * bit 0 of factor_cache_valid is 0, reused when it is 1 -- the caller flips the flag and invalidates it when
   * Z / sigma / lengthscale / group parameters / jitter change (SURVEY §8f "next" #3).  Behind the factor the
   * buffer keeps what the two products need of q(U) (LuE^T, muE, un-whitened LuE) as the LAST call prepared it from
   * (mu, Lu_raw); bit 1 (factor_cache_valid == 3) tells gpz_svgp_backward that this is the very (mu, Lu_raw) it is
   * called with -- the backward pass of the forward that wrote the buffer -- so it is not prepared a second time. */
  void* factor_cache;
  int64_t factor_cache_valid;
  /* Optional retained Wt = Linv Kzx of every N-chunk plus its column-sum partials, for training:
   * non-NULL (gpz_svgp_wt_cache_bytes bytes, caller owned) makes gpz_svgp_forward write them there;
   * gpz_svgp_backward with wt_cache_valid != 0 (same inputs, same `chunk`) reads them instead of
   * rebuilding Kzx and repeating the first triangular product (one of its three big GEMMs). */
  void* wt_cache;
  int64_t wt_cache_valid;
} gpz_svgp_problem;

size_t gpz_svgp_factor_cache_bytes(const gpz_svgp_problem* p);
size_t gpz_svgp_wt_cache_bytes(const gpz_svgp_problem* p, int64_t chunk);

size_t gpz_svgp_workspace_bytes(const gpz_svgp_problem* p, int64_t chunk);
/* Which kernels gpz_svgp_forward takes for the two big products of this problem and chunk (0 = automatic chunk):
 * bit 0 the wide-tile fp32 kernels, bit 1 the generated-Kzx stage 1; 4: the panel kernel (both products in one launch);
 * 0: the 128 x 128-tile kernels; -1: bad problem.
 * Unknown bits in `flags` are an error since ABI 210 (the word was `reserved` before 200: zero it). */
int gpz_svgp_forward_path(const gpz_svgp_problem* p, int64_t chunk);
int gpz_svgp_forward(const gpz_svgp_problem* p, int64_t chunk, void* ws, size_t ws_bytes,
                     void* stream);

/* Backward of gpz_svgp_forward: given dLoss/dmean and dLoss/dscale of q(F) (and the forward's
 * scale) writes dLoss/dmu (L,M) and dLoss/dLu_raw (L,M,M) -- what torch autograd produces through
 * gp.py:276-296 / 218-228 for loss.backward() (utilities.py:485) with frozen kernel
 * hyper-parameters (the training mode of Slideseq_NSF_newest_version.ipynb:500-504) -- and,
 * optionally, the gradients w.r.t. sigma / lengthscale / group parameter and Z.  Same problem
 * description as the forward; its output fields are ignored. */
typedef struct gpz_svgp_grads {
  const void* g_mean;    /* (L,N) dtype */
  const void* g_scale;   /* (L,N) dtype */
  const void* scale;     /* (L,N) dtype: forward output */
  void* grad_mu;         /* (L,M) dtype */
  void* grad_Lu_raw;     /* (L,M,M) dtype, zeros above the diagonal */
  /* optional: gradients w.r.t. the kernel hyper-parameters and the inducing inputs -- what
   * autograd sends through kernel.forward, cholesky and the solves (kernels.py, gp.py:213-219,
   * 270-276).  NULL: frozen hyper-parameters. */
  double* grad_theta;    /* (L,4) fp64: d/dsigma, d/dlengthscale, d/dgroup_a (effective), 0 */
  double* grad_Z;        /* (M,4) fp64: first d columns used */
  const void* g_chol;    /* (L,M,M) dtype or NULL: upstream dLoss/dchol (un-whitened: KL(qU||pU) uses it) */
  /* (L,) fp64 or NULL: upstream dLoss/dkl_l of the per-latent KL the forward pass reports (`kl`).  The
   * KL's own gradient -- kl_divergence(qU, pU) through torch's MVN KL and its autograd in the reference
   * (utilities.py:481) -- is then folded into grad_mu, grad_Lu_raw and, with grad_theta / grad_Z, into
   * the factor's gradient, at no extra matrix product: dKL/dLuE = LuE, dKL/dmuE = muE, plus the
   * log-determinant diagonals (whitened: LuE = Lu, muE = mu, the whitened_KL of utilities.py:27-36). */
  const double* g_kl;
  /* gpz_vnngp_backward only: (N,) int64 permutation of the points, or NULL (identity).  The pass lays its per-point
   * records out in this order; along a space-filling curve the points that share an inducing point are neighbours in
   * memory, which is what its fixed-order gather is bound by.  Any permutation gives the same sums up to the order of
   * their terms (the order is fixed by the permutation: results stay bitwise reproducible). */
  const int64_t* point_order;
} gpz_svgp_grads;

size_t gpz_svgp_backward_workspace_bytes(const gpz_svgp_problem* p, int64_t chunk);
int gpz_svgp_backward(const gpz_svgp_problem* p, const gpz_svgp_grads* g, int64_t chunk, void* ws,
                      size_t ws_bytes, void* stream);

/* Monte-Carlo expected Poisson log-likelihood of the NSF factor models and its gradients, fused
 * (SURVEY §8f "next" #2): replaces get_rate + Poisson(V*Z).log_prob(y).mean(0).sum() and their
 * autograd (likelihoods.py:49-53, 74-97, 199-225; utilities.py:610-616) without materialising the
 * (E,D,N) rate.  fp32.  mean, scale (Lt,N): q(F) moments of all factors; eps (E,Lt,N): the
 * standard-normal draws of rsample; W (D,Lt), V (N,): POSITIVE loadings / size factors (after
 * softplus); y (D,N) counts.  Outputs: loglik (2,) fp64: [0] = (1/E) sum_e sum_dn [y log(VZ) - VZ],
 * [1] = sum_dn lgamma(y+1) (0 unless with_lgamma; Poisson.log_prob = [0] - [1]); and
 * d loglik[0] / d{mean, scale, W, V}.  Lt <= 64 factors; E <= 32 samples per call (more samples: one call per group
 * of 32, as gpzoo_amd/ops.py does; y is read once per pass whatever E is).  The three dense products (rate, dW,
 * d exp F) run on MFMA.
 * Alignment: every array argument (the six inputs, the five outputs) and ws must be 16-byte aligned -- rows of y and of
 * the partial-sum slabs are read and written 16 bytes at a time from the base pointers on whenever N % 4 == 0.  A
 * misaligned pointer is an argument error on the host, before any launch (hipMalloc and torch allocations are
 * aligned; a view at an element offset need not be: gpzoo_amd/ops.py copies such inputs). */
size_t gpz_poisson_nsf_workspace_bytes(int64_t N, int64_t D, int32_t Lt, int32_t E);
int gpz_poisson_nsf(const float* mean, const float* scale, const float* eps, const float* W,
                    const float* V, const float* y, int64_t N, int64_t D, int32_t Lt, int32_t E,
                    int32_t with_lgamma, double* loglik, float* dmean, float* dscale, float* dW,
                    float* dV, void* ws, size_t ws_bytes, void* stream);

/* gpz_poisson_nsf under a negative-binomial likelihood (csrc/nb.hip), torch's parameterisation:
 * NegativeBinomial(total_count = theta[d], logits = log mu - log theta[d]) with mu = V[n] sum_l W[d,l] exp(F[e,l,n]), so
 * the variance is mu + mu^2 / theta and theta -> infinity is the Poisson step.  theta (D,) positive joins W as a per-gene
 * operand and dtheta (D,) the gradients; every other argument is as in gpz_poisson_nsf, the mean over E applied.
 * loglik[0] = (1/E) sum_{e,d,n} [ y log(mu / (mu + theta)) - theta log1p(mu / theta) + lgamma(y + theta) - lgamma(theta) ],
 * loglik[1] = sum_{d,n} lgamma(y + 1) (0 when with_lgamma == 0): the log-likelihood is loglik[0] - loglik[1].
 * fp32, the three dense products on v_mfma_f32_16x16x4_f32, log1p compensated, the terms in y and theta alone summed per
 * gene in fp64 by a pass of their own; the (E, D, N) rate never reaches memory and the workspace holds nothing of D x N
 * elements.  No floating-point atomics, every sum in a fixed order: two calls agree bit for bit.
 * 1 <= Lt <= 64, 1 <= E <= 32 per call, D < 2^31, E Lt N < 2^29; N need not be a multiple of 4.  Every array argument and
 * ws must be 16-byte aligned.  Argument errors (null pointers, extents, Lt, E, a small workspace, alignment) return -1
 * before any launch; the workspace query then returns 0 and leaves the reason in gpz_last_error.
 * gpz_nb_nsf_plan (host only, no device needed; any out pointer may be NULL): factors_padded = Lt rounded up to the
 * kernel instance, aligned_rows = 1 when N % 4 == 0 (rows of y and of the slabs move 16 bytes at a time), gene_slices and
 * spot_slices = partial slabs of the spot pass and of the gene pass. */
int gpz_nb_nsf_plan(int64_t N, int64_t D, int32_t Lt, int32_t E, int32_t* factors_padded, int32_t* aligned_rows,
                    int32_t* gene_slices, int32_t* spot_slices);
size_t gpz_nb_nsf_workspace_bytes(int64_t N, int64_t D, int32_t Lt, int32_t E);
int gpz_nb_nsf(const float* mean, const float* scale, const float* eps, const float* W, const float* V,
               const float* theta, const float* y, int64_t N, int64_t D, int32_t Lt, int32_t E, int32_t with_lgamma,
               double* loglik, float* dmean, float* dscale, float* dW, float* dV, float* dtheta, void* ws,
               size_t ws_bytes, void* stream);

/* The Gaussian member of the family (csrc/gaussian.hip): real-valued y (D,N), real loadings W (D,Lt), intercept b (D,) and
 * one noise standard deviation per gene, noise_sd (D,) > 0 (a scale, not a variance), under q(F) = N(mean, scale^2)
 * independent with mean and scale (Lt,N).  This is the likelihood of RSF (a GP prior on F; the nsf paper's
 * real-valued spatial factorisation, MEFISTO's model) and of FA (an i.i.d. prior).  There is no link function, so the
 * expectation under q(F) has a closed form -- no samples, no eps, an exact value:
 *   r = y - b - W mean,  R[d] = sum_n r^2,  S[l] = sum_n scale^2,  Q[d] = sum_l W[d,l]^2 S[l]
 *   loglik[0]       = sum_d [ -N (log(2 pi) / 2 + log noise_sd[d]) - (R[d] + Q[d]) / (2 noise_sd[d]^2) ]
 *   sse_per_gene[d] = R[d]  (fp64; the squared error of the predictive mean; may be NULL)
 *   dmean = W^T g with g = r / noise_sd^2,  dscale[l,n] = -scale[l,n] sum_d W[d,l]^2 / noise_sd[d]^2,
 *   dW = g mean^T - W S / noise_sd^2,  db = sum_n g,  dnoise_sd = -N / noise_sd + (R + Q) / noise_sd^3
 * Several factor sets concatenate along Lt as in the count steps.  fp32 operands, the dense products on
 * v_mfma_f32_16x16x4_f32, every sum across tiles fp64 in a fixed order, no floating-point atomics: two calls agree bit
 * for bit.  y is read twice by a gradient call and once by a value-only call: the five gradient pointers are either
 * all set or all NULL, and with all NULL only loglik and sse_per_gene are computed (held-out scoring).
 * The scratch memory is the explicit argument `partials` (partial sums per gene slice and spot slice; nothing of D x N
 * elements); it need not be cleared and may hold anything.  Its size comes from the host-only plan query, which also
 * reports factors_padded (Lt rounded up to the kernel instance), aligned_rows (1 when N % 4 == 0: rows of y and of the
 * slabs move 16 bytes at a time), gene_slices and spot_slices (any out pointer may be NULL).
 * Supported range of noise_sd: 1e-18 <= noise_sd[d] <= 1e18 (finite).  The spot pass forms 1 / noise_sd^2 in fp32, which
 * overflows to inf below about 5e-20 and flushes towards 0 above about 2e19: dmean then holds inf / NaN or zeros while the
 * outputs the finish kernel forms in fp64 (loglik, sse_per_gene, dW, db, dnoise_sd) stay finite.  The values are not checked
 * (that would need a pass over device memory); a caller that trains noise_sd keeps it inside the range.
 * 1 <= Lt <= 64, 1 <= N, D < 2^31; N need not be a multiple of 4.  Every array argument and partials must be 16-byte
 * aligned.  Argument errors (a null among the inputs, loglik or partials, gradient pointers partly set, extents, Lt, a
 * small partials_bytes, alignment) return -1 before any launch; the plan query then returns a negative value and leaves
 * the reason in gpz_last_error. */
int gpz_gaussian_fa_plan(int64_t N, int64_t D, int32_t Lt, int32_t* factors_padded, int32_t* aligned_rows,
                         int32_t* gene_slices, int32_t* spot_slices, int64_t* partials_bytes);
int gpz_gaussian_fa(const float* mean, const float* scale, const float* W, const float* b, const float* noise_sd,
                    const float* y, int64_t N, int64_t D, int32_t Lt, double* loglik, double* sse_per_gene,
                    float* dmean, float* dscale, float* dW, float* db, float* dnoise_sd,
                    void* partials, size_t partials_bytes, void* stream);

/* gpz_gaussian_fa for expression stored as its non-zeros minus a per-gene offset (csrc/gaussian_sparse.hip):
 *   y[d,n] = z[d,n] - offset[d],
 * where z is held in the two orders of gpz_poisson_nsf_sparse below (col_ptr, col_gene, col_val by spot; row_ptr, row_spot,
 * row_perm by gene; the same trust in the arrays) -- log1p of size-normalised counts, centred per gene, is of this form
 * and z then has exactly the sparsity of the counts.  The expected log-likelihood is quadratic in y, so the offset folds
 * into the intercept: with a = b + offset, iv = 1 / noise_sd^2, p[d,n] = a[d] + W[d,:] . mean[:,n], M1 = sum_n mean[:,n],
 * G = sum_n mean[:,n] mean[:,n]^T, S2[l] = sum_n scale[l,n]^2, u = sum_d iv a W[d,:], H = sum_d iv W[d,:] W[d,:]^T,
 *   sse_per_gene[d] = sum_nz(d) z (z - 2 p) + B a^2 + 2 a W[d,:] . M1 + W[d,:] G W[d,:]^T      R[d] = sse + sum_l W[d,l]^2 S2[l]
 *   loglik[0]       = sum_d [ -B (log(2 pi) / 2 + log noise_sd[d]) - iv R[d] / 2 ]
 *   ss_per_gene[d]  = sum_nz(d) z^2 - (sum_nz(d) z)^2 / B    (fp64; the null sum of squares of R^2, the offset cancels)
 *   dmean[:,n] = sum_nz(n) iv z W[d,:] - u - H mean[:,n],  dscale[l,n] = -scale[l,n] H[l,l],
 *   dW[d,:] = iv [ sum_nz(d) z mean[:,n] - a M1 - G W[d,:] - S2 * W[d,:] ],  db[d] = iv [ sum_nz(d) z - B a - W[d,:] . M1 ],
 *   dnoise_sd[d] = -B / noise_sd + R[d] / noise_sd^3
 * -- the numbers of gpz_gaussian_fa on the dense (D,B) array, for O(nnz_B Lt + (B + D) Lt^2) work; nothing of D x B or nnz
 * elements is read, written or allocated beyond the stored entries themselves.  mean, scale (Lt,B), W (D,Lt), b, noise_sd
 * (D,) fp32; offset (D,) fp64.  idx (B) lists the batch's distinct spots and pos (N) is its inverse (-1 outside the batch);
 * both NULL: the whole data set, B = N.  sse_per_gene and ss_per_gene may be NULL.  The five gradient pointers are either
 * all set or all NULL (value-only: loglik, sse_per_gene and ss_per_gene, the same bits as in a gradient call).
 * Every accumulation and the quadratic terms are fp64 in a fixed order, no atomics: two calls agree bit for bit.  The
 * scratch memory is the explicit argument `partials` as for gpz_gaussian_fa; it need not be cleared and may hold anything.
 * Its size is the plan query's workspace_bytes; the plan (host only, any out pointer may be NULL) also reports gene_chunk
 * (stored entries of a gene row per wave of the gene pass), n_gene_chunks (the bound D + nnz / gene_chunk on the length of
 * its work list) and factors_padded (Lt rounded up to the kernel instance).
 * 1 <= Lt <= 64, 1 <= B <= N, N, D, nnz < 2^31; noise_sd as for gpz_gaussian_fa.  The inputs need only their natural alignment,
 * partials 16 bytes.  Argument errors return -1 before any launch with the reason in gpz_last_error. */
int gpz_gaussian_fa_sparse_plan(int64_t N, int64_t B, int64_t D, int32_t Lt, int64_t nnz, int32_t* gene_chunk,
                                int64_t* n_gene_chunks, int32_t* factors_padded, int64_t* workspace_bytes);
int gpz_gaussian_fa_sparse(const float* mean, const float* scale, const float* W, const float* b, const float* noise_sd,
                           const double* offset, const int64_t* col_ptr, const int32_t* col_gene, const float* col_val,
                           const int64_t* row_ptr, const int32_t* row_spot, const int32_t* row_perm,
                           const int32_t* idx, const int32_t* pos, int64_t N, int64_t B, int64_t D, int64_t nnz,
                           int32_t Lt, double* loglik, double* sse_per_gene, double* ss_per_gene, float* dmean,
                           float* dscale, float* dW, float* db, float* dnoise_sd, void* partials,
                           size_t partials_bytes, void* stream);

/* Per-gene scores of a whole data set stored as its non-zeros (csrc/gene_rank.hip), read in the by-gene order of
 * gpz_poisson_nsf_sparse below: row_ptr int64 (D + 1), row_spot int32 (nnz), row_perm int32 (nnz), the value of entry k being
 * col_val[row_perm[k]], fp32 (the same trust in the arrays; an index outside its range is skipped, never dereferenced).  The
 * reference's anndata_to_train_val takes genes "sorted in decreasing importance (eg with deviance)" as a precondition
 * (utilities.py:192-230) and computes neither score.  All outputs are fp64 arrays of D values, fully written.
 *
 * gpz_gene_deviance_sparse: size (N,) fp64, > 0 wherever a spot has a stored entry; S = sum_n size[n] is formed inside.
 *   sum[d] = sum_nz y,  count[d] = the stored entries of gene d,  p = sum / S,
 *   family 0 (Poisson):   deviance[d] = 2 [ sum_nz y log(y / size_n) - sum log(sum / S) ]
 *   family 1 (binomial):  deviance[d] = 2 [ sum_nz ( y log(y / size_n) + (size_n - y) log1p(-y / size_n) )
 *                                           - sum (log p - log1p(-p)) - S log1p(-p) ]        (size = the spot's total, y <= size)
 * A term with y == size_n is y log 1 + 0 = 0 (scry's na.rm=TRUE), as is the null term at p == 1; a gene with no stored
 * entry has deviance 0.  All logs are fp64.
 *
 * gpz_gene_morans_i_sparse: nbr (N,K) int64, 1 <= K <= 32, K < N.  I[d] = gpz_morans_i of column d of the dense transpose
 * (zeros included, row-normalised weights 1 / K), from the expanded form: S = sum x, Q = sum x^2, xbar = S / N,
 *   C = sum_{i in nz} x_i sum_{j in nbr(i)} x_j,   A = sum_{i in nz} indeg(i) x_i,
 *   I = [ C - xbar (K S + A) + N K xbar^2 ] / ( K (Q - N xbar^2) ).
 * NaN for a gene with no stored entry, for a gene stored at every spot with one single value (found from count, min and
 * max, not from the cancelled denominator) and wherever the denominator is <= 0.  A nearly constant gene loses digits in
 * proportion to mean^2 / variance.  The in-degree of the table is counted once per call, in the scratch memory.  Each
 * entry of nbr is checked on the device as by gpz_morans_i: one outside [0, N) or equal to its row is not read, not counted,
 * and info[0] (device int32) is set to 1.
 *
 * Every accumulation is fp64 in a fixed order with no atomics on values (the in-degree histogram uses integer atomics): two
 * calls agree bit for bit.  The scratch memory is the explicit argument `partials` as for gpz_gaussian_fa_sparse; it need not
 * be cleared and may hold anything.  Its size is the plan query's partials_bytes; the plan (host only, any out pointer may
 * be NULL) also reports gene_chunk (stored entries of a gene row per sweep of its workgroup) and workgroups (genes in
 * flight; the Moran scratch is workgroups x N x 4 bytes plus N x 4, independent of D beyond that).  Nothing of D x N or nnz
 * elements is allocated.  N, D, nnz < 2^31; partials 16-byte aligned.  Argument errors return -1 before any launch with the
 * reason in gpz_last_error. */
int gpz_gene_deviance_sparse_plan(int64_t N, int64_t D, int64_t nnz, int32_t* gene_chunk, int32_t* workgroups,
                                  int64_t* partials_bytes);
int gpz_gene_deviance_sparse(const int64_t* row_ptr, const int32_t* row_spot, const int32_t* row_perm, const float* col_val,
                             const double* size, int64_t N, int64_t D, int64_t nnz, int32_t family, double* sum,
                             double* count, double* deviance, void* partials, size_t partials_bytes, void* stream);
int gpz_gene_morans_i_sparse_plan(int64_t N, int64_t D, int64_t nnz, int32_t K, int32_t* gene_chunk, int32_t* workgroups,
                                  int64_t* partials_bytes);
int gpz_gene_morans_i_sparse(const int64_t* row_ptr, const int32_t* row_spot, const int32_t* row_perm, const float* col_val,
                             const int64_t* nbr, int64_t N, int64_t D, int64_t nnz, int32_t K, double* I, int32_t* info,
                             void* partials, size_t partials_bytes, void* stream);

/* Gene-wise negative-binomial inverse dispersion by maximum likelihood (csrc/gene_dispersion.hip), over the same by-gene
 * arrays as the two entries above, fp64 throughout.  Null of gene d: mu_n = p_d size_n, p_d = sum_n y_dn / sum_n size_n (the
 * null of gpz_gene_deviance_sparse and gpz_nb_deviance; the rate's MLE for constant sizes, a convention otherwise).  theta[d]
 * maximises l_d(theta) = sum_n log NB(y_dn | mu_n, theta) over [theta_min, theta_max]: the root in t = log theta of
 *   S_d(t) = sum_{all n} theta h(mu_n / theta) + sum_{stored} theta sum_{k < y} (mu_n - k) / ((theta + k)(theta + mu_n)),
 *   h(x) = x / (1 + x) - log1p(x),
 * found by Newton steps in t kept inside a sign-changing bracket (bisection otherwise), from the moment estimate
 *   theta_0 = sum_n mu_n^2 / (sum_n (y_n - mu_n)^2 - sum_n y_n), theta_max where the denominator is <= 0, clipped into the
 * range; it stops at a step or bracket <= tol_t (the plan reports it: 1e-9) or after max_iter <= 200 score evaluations.
 *   theta[d]           the root (status 0); +inf when S_d(log theta_max) >= 0 (1: no overdispersion in range); theta_min when
 *                      S_d(log theta_min) <= 0 (2); the last iterate, theta_0 for max_iter = 0, when not converged (3);
 *                      NaN for a gene without counts (4)
 *   gain[d]            l_d(theta[d]) - l_d(inf) = sum_{all n} [mu_n - theta log1p(mu_n / theta)]
 *                      + sum_{stored} sum_{k < y} log((theta + k) / (theta + mu_n)); exactly 0 at status 1 and 4
 *   poisson_loglik[d]  l_d(inf) = sum_{stored} [y log mu_n - lgamma(y + 1)] - sum_n y_dn; 0 at status 4
 *   status[d], iterations[d]  int32; iterations counts the score evaluations after the two at the ends of the range
 * Every term is evaluated without cancellation inside it (series for small mu / theta, explicit sums over k below 16 and the
 * combined difference of the psi / lgamma asymptotic series above: csrc/gene_dispersion.hip).  size (N,) fp64 >= 0 and > 0
 * wherever a spot has a stored count; a spot of size 0 contributes nothing.  When all sizes are equal (found once per call)
 * the all-spot sums are N f(x) and no sweep over the spots is made.  A stored value that is negative, not an integer or
 * >= 2^24 is not used and sets bit 0 of info[0] (device int32); a negative or non-finite size, or a stored count at a spot
 * of size 0, is not used and sets bit 1.  Every accumulation is fp64 in a fixed order with no atomics on values: two calls
 * agree bit for bit.  The scratch is `partials` (four fp64 words, whatever the shape), sized by the host-only plan query,
 * which also reports gene_chunk, workgroups and tol_t (any out pointer may be NULL); it need not be cleared.  Nothing of
 * D x N or nnz elements is allocated.  N, D, nnz < 2^31; partials 16-byte aligned.  Argument errors (null pointers, bad
 * extents, a range that is not 0 < theta_min < theta_max finite, max_iter outside [0, 200], misaligned or short partials)
 * return -1 before any launch with the reason in gpz_last_error. */
int gpz_gene_dispersion_sparse_plan(int64_t N, int64_t D, int64_t nnz, int32_t* gene_chunk, int32_t* workgroups,
                                    double* tol_t, int64_t* partials_bytes);
int gpz_gene_dispersion_sparse(const int64_t* row_ptr, const int32_t* row_spot, const int32_t* row_perm, const float* col_val,
                               const double* size, int64_t N, int64_t D, int64_t nnz, double theta_min, double theta_max,
                               int32_t max_iter, double* theta, double* gain, double* poisson_loglik, int32_t* status,
                               int32_t* iterations, int32_t* info, void* partials, size_t partials_bytes, void* stream);

/* The sparse-GP test for spatially variable genes (csrc/gene_gp.hip; gpzoo.utilities.gene_spatial_gp assembles it), fp64
 * throughout.  One gene is y (N,), a row of centred expression; the model y = f + eps, f ~ GP(0, s k_l), eps ~ N(0, tau I) with a
 * unit-variance stationary kernel k_l and inducing points Z (M, d) is scored by Titsias' collapsed bound.  With Lz = chol(K_zz +
 * jitter I), Phi = Lz^-1 K_zx, B = Phi Phi^T = U diag(lam) U^T, p = U^T Phi y, delta = tau / s and s profiled out:
 *   Q(delta) = y.y - sum_i p_i^2 / (delta + lam_i),   R = Q / delta,   s = R / N,   tau = s delta,
 *   F(delta) = -1/2 [ N log 2 pi + N log(R / N) + N + (N - M) log delta + sum_i log(delta + lam_i) + (N - sum_i lam_i) / delta ],
 * which tends to the null model's F_0 = -1/2 N (log(2 pi y.y / N) + 1) as delta -> inf.
 *
 * gpz_gene_kernel_project_sparse: out[l, g, m] = sum_{stored (g, n)} v_gn k_l(z_m, x_n), out (n_ell, D, M) -- K_zx Y^T of every
 * gene of a WHOLE data set stored as its non-zeros (the by-gene arrays of gpz_gene_deviance_sparse; the centring is the
 * caller's: K_zx y = K_zx z - offset K_zx 1), for n_ell length scales (device array, fp64), X (N, d) and Z (M, d) fp64 device
 * arrays, 1 <= d <= 4, 1 <= M <= 1024, 1 <= n_ell <= 16, kind GPZ_KERNEL_RBF, _MATERN12, _MATERN32 or _MATERN52.  The covariances
 * are generated in the kernel with the fp64 operations of gpz_kernel_gram at sigma = 1 (the same bits) and never stored: nothing
 * of N x M or nnz elements is allocated.  The distance of a pair is computed once for all length scales.  A row longer than
 * gene_chunk entries (the plan: a multiple of 256, at least N / 4) is cut into chunks of that many; a sum runs over the
 * entries of a chunk in row order, each term the rounded product added to the running sum, then over the chunks in order: it
 * depends on N (through gene_chunk) and on nothing else -- not on `workgroups` (0: the plan's; any value up to 65535 gives the
 * same bits).  No atomics.  An entry whose spot or position is out of range counts as a stored zero.  The scratch is `partials`
 * (the sums of the chunks after a row's first: nnz / gene_chunk + 1 slots of n_ell x M values), sized by the plan query; it
 * need not be cleared.  The plan's `generate` is 1 while this entry is the faster way to the result and 0 above 290 N stored
 * entries, where filling K_xz per length scale (gpz_kfill) and gathering its rows (gpz_counts_matmul) costs less than the
 * exp per (entry, inducing point, length scale) generated here (measured on an MI355X; csrc/gene_gp.hip has the figures); the
 * entry computes either way.
 *
 * gpz_gene_gp_profile: per (gene, length scale) the maximum of F over t = log delta in [log delta_min, log delta_max].  p (n_ell,
 * D, M), lam (n_ell, M) >= 0, yty (D,) = y.y, device arrays.  F is evaluated on a uniform grid of grid_points (33) values of t;
 * the best point, ties to the lower index, starts a Newton iteration on dF/dt between its two grid neighbours, kept inside a
 * bracket and bisecting when a step leaves it or does not halve the derivative; it stops at a step or bracket <= tol_t (1e-9)
 * or after max_iter (100) evaluations.  Outputs (D, n_ell): loglik = F at the optimum, delta, s2 = R / N, tau2 = s2 delta there,
 * status int32 (0 interior; 1 the best grid point is the last and F still rises there: no spatial variance in range, the
 * values at delta_max; 2 the best is the first and F falls from there: the lower bound; 3 degenerate: y.y <= 0 or not finite,
 * or Q <= 0 or F not finite on the grid -- NaN in the four values) and iterations int32 (evaluations after the grid; max_iter:
 * not converged).  One wave per pair, every sum in a fixed order: two calls agree bit for bit.  No scratch.
 *
 * Argument errors (null pointers, extents or limits above, a bad kind or delta range, misaligned or short partials) return -1
 * before any launch with the reason in gpz_last_error.  The plan queries are host-only; any out pointer may be NULL. */
int gpz_gene_kernel_project_sparse_plan(int64_t N, int64_t D, int64_t nnz, int64_t M, int32_t n_ell, int32_t* gene_chunk,
                                        int32_t* workgroups, int32_t* generate, int64_t* partials_bytes);
int gpz_gene_kernel_project_sparse(const int64_t* row_ptr, const int32_t* row_spot, const int32_t* row_perm, const float* col_val,
                                   const double* X, const double* Z, const double* lengthscales, int64_t N, int64_t D, int64_t nnz,
                                   int64_t M, int32_t d, int32_t n_ell, int32_t kind, int32_t workgroups, double* out,
                                   void* partials, size_t partials_bytes, void* stream);
int gpz_gene_gp_profile_plan(int64_t D, int64_t M, int32_t n_ell, int32_t* grid_points, int32_t* workgroups, double* tol_t,
                             int32_t* max_iter);
int gpz_gene_gp_profile(const double* p, const double* lam, const double* yty, int64_t N, int64_t D, int64_t M, int32_t n_ell,
                        double delta_min, double delta_max, double* loglik, double* delta, double* s2, double* tau2,
                        int32_t* status, int32_t* iterations, void* stream);

/* Moran's I of every gene under P relabellings of the spots (csrc/moran_perm.hip): the permutation null of squidpy's
 * spatial_autocorr(..., n_perms=) and of PySAL's Moran.  perms (P, N) int32, row p a permutation pi of 0 .. N - 1; the permuted
 * gene is x^pi[i] = x[pi[i]], scored over the fixed table nbr (N, K) int64, 1 <= K <= 32, K < N, weights 1 / K.  The graph is
 * relabelled, not the values: T_pi[pi[i], m] = pi[nbr[i, m]] and indeg_pi[pi[i]] = indeg[i] go to the scratch memory for a
 * batch of perm_batch permutations at a time, and in the expansion of gpz_gene_morans_i_sparse only
 *   C_pi = sum_{i stored} x_i sum_m x[T_pi[i, m]]   and   A_pi = sum_{i stored} indeg_pi(i) x_i
 * depend on pi: O(entries x K) per permutation, nothing of D x N elements is formed.
 *   gpz_gene_morans_perm_sparse  the by-gene arrays of a WHOLE data set stored as its non-zeros, as gpz_gene_morans_i_sparse
 *   gpz_morans_perm_rows         values fp32 (D, N), contiguous: every spot is an entry, zeros included
 * Outputs, fp64 (D,) unless said otherwise:
 *   I         gpz_gene_morans_i_sparse's I of the unpermuted gene, bit for bit (the rows entry: the same expansion over all N
 *             spots); NaN as there
 *   sims      (D, P), may be NULL: I_pi, the same expression on (S, Q, C_pi, A_pi); a row of perms that is the identity gives
 *             I, bit for bit
 *   n_ge, n_le   int32: the permutations with I_pi >= I and with I_pi <= I, decided on t = N C - S A in fp64 (the numerator
 *             is C - S A / N and the denominator does not depend on pi).  Exact for integer-valued data with |t| < 2^53:
 *             ties are then counted as ties on every run and every path; for other data a mathematical tie may fall
 *             either way in the last bit.  0 for a gene whose I is NaN
 *   sim_mean, sim_m2   mean of I_pi over the P permutations and sum (I_pi - mean)^2, by Welford's update in permutation
 *             order; NaN where I is
 * info[0] (device int32): 1 when an entry of nbr lies outside [0, N) or names its own row (as gpz_gene_morans_i_sparse), 2 when
 * a row of perms is no permutation (an entry outside [0, N), or an index named twice); such entries are skipped, nothing is
 * read or written out of range, and the outputs are then meaningless.
 * line_mode: where a gene's line of N floats lives while its permutations are evaluated -- 1 the scratch memory, 2 the
 * workgroup's LDS (an argument error unless 4 N + 512 <= 163840 bytes), 0 = the plan's choice: LDS wherever it fits.
 * perm_batch: permutations per launch, at most 32; 0 = the plan's choice: the tables of a batch take at most 256 MiB, at
 * most P, and at most 16 with the line in LDS (one permutation per wave of the workgroup) or 8 with the line in the scratch
 * memory (more tables in flight cost time there).  Every sum is fp64 in
 * a fixed order with no atomics on values (integer atomics count the in-degree and the writes of the relabelling): all
 * outputs are reproducible bit for bit and independent of perm_batch and line_mode.  The scratch is `partials`, sized by the
 * host-only plan query (any out pointer may be NULL), which reports perm_batch and line_mode as resolved, workgroups (genes
 * in flight) and partials_bytes; it need not be cleared.  N, D, nnz, P < 2^31, P >= 1; partials 16-byte aligned.  Argument
 * errors return -1 before any launch with the reason in gpz_last_error. */
int gpz_gene_morans_perm_sparse_plan(int64_t N, int64_t D, int64_t nnz, int32_t K, int64_t P, int32_t perm_batch_wanted,
                                     int32_t line_mode_wanted, int32_t* perm_batch, int32_t* line_mode, int32_t* workgroups,
                                     int64_t* partials_bytes);
int gpz_gene_morans_perm_sparse(const int64_t* row_ptr, const int32_t* row_spot, const int32_t* row_perm, const float* col_val,
                                const int64_t* nbr, const int32_t* perms, int64_t N, int64_t D, int64_t nnz, int32_t K, int64_t P,
                                int32_t perm_batch, int32_t line_mode, double* I, double* sims, int32_t* n_ge, int32_t* n_le,
                                double* sim_mean, double* sim_m2, int32_t* info, void* partials, size_t partials_bytes,
                                void* stream);
int gpz_morans_perm_rows_plan(int64_t N, int64_t D, int32_t K, int64_t P, int32_t perm_batch_wanted, int32_t line_mode_wanted,
                              int32_t* perm_batch, int32_t* line_mode, int32_t* workgroups, int64_t* partials_bytes);
int gpz_morans_perm_rows(const float* values, const int64_t* nbr, const int32_t* perms, int64_t N, int64_t D, int32_t K, int64_t P,
                         int32_t perm_batch, int32_t line_mode, double* I, double* sims, int32_t* n_ge, int32_t* n_le,
                         double* sim_mean, double* sim_m2, int32_t* info, void* partials, size_t partials_bytes, void* stream);

/* Moran's I, Geary's C and the moments of every gene (csrc/spatial_stats.hip, csrc/moran_expr.h).  Over the table nbr (N, K) int64
 * of distinct neighbours without self edges, with binary weights (both ratios are the same for weights 1 / K):
 *   C = (N - 1) G / ( 2 N K sum_i (x_i - xbar)^2 ),   G = sum_i sum_{j in nbr(i)} (x_i - x_j)^2,
 * 1 in expectation, below 1 for positive autocorrelation.  Outputs, fp64, one value per gene / column; each of the five may be
 * NULL and is then not computed:
 *   I          gpz_gene_morans_i_sparse's / gpz_morans_i's, bit for bit
 *   C          Geary's C
 *   mean, var  xbar and m2 = sum (x - xbar)^2 / N (zeros included)
 *   kurtosis   b2 = m4 / m2^2, m4 = sum (x - xbar)^4 / N: what the randomisation variances of I and C (Cliff & Ord; PySAL's
 *              VI_rand, VC_rand) depend on beside the graph
 * gpz_gene_spatial_stats_sparse: the by-gene arrays of a WHOLE data set stored as its non-zeros and 1 <= K <= 32, K < N, as
 * gpz_gene_morans_i_sparse, one workgroup per gene at a time over the same line of N floats.  With its sums S, Q, C_s and
 *   Q_in = sum_{i stored} indeg(i) x_i^2:   G = K Q + Q_in - 2 C_s,   C = (N - 1) G / ( 2 N K (Q - N xbar^2) );
 * a constant added to every spot of a gene leaves G as it is.  A nearly constant gene loses digits in proportion to
 * mean^2 / variance, in G as in the denominator.  mean = S / N; var and kurtosis come from a second sweep of the row,
 *   m_k = [ sum_{stored} (x - xbar)^k + (N - stored) xbar^k ] / N, sums of non-negative terms.  I, C and kurtosis are NaN for
 * a gene without stored entries and for a gene stored at every spot with one single value, and I and C wherever the
 * denominator is <= 0 (gpz_gene_morans_i_sparse's rule); mean and var are 0 and the value for those.
 * gpz_spatial_stats: the first L columns of values (N, L), fp32 or fp64 (dtype), 1 <= K < N, as gpz_morans_i takes them, in its
 * arithmetic: z = v - mean, G = sum_i sum_j (z_i - z_j)^2 a sum of non-negative terms, var = sum z^2 / N, m4 = sum z^4 / N.  A
 * constant column gives NaN in I, C and kurtosis (0 / 0).
 * info[0] (device int32) is set to 1 by an entry of nbr outside [0, N) or naming its own row, which is not read and not
 * counted.  Every accumulation is fp64 in a fixed order with no atomics on values: two calls agree bit for bit.  The scratch is
 * `partials`, sized by the host-only plan query (any out pointer may be NULL), and need not be cleared: workgroups x N x 4 + N x 4
 * bytes for the sparse entry (gene_chunk, workgroups as gpz_gene_morans_i_sparse_plan), 40 bytes per chunk of row_chunk rows
 * and column plus 8 per column for the other.  Nothing of D x N or nnz elements is allocated.  partials 16-byte aligned.
 * Argument errors return -1 before any launch with the reason in gpz_last_error. */
int gpz_gene_spatial_stats_sparse_plan(int64_t N, int64_t D, int64_t nnz, int32_t K, int32_t* gene_chunk, int32_t* workgroups,
                                       int64_t* partials_bytes);
int gpz_gene_spatial_stats_sparse(const int64_t* row_ptr, const int32_t* row_spot, const int32_t* row_perm, const float* col_val,
                                  const int64_t* nbr, int64_t N, int64_t D, int64_t nnz, int32_t K, double* I, double* C, double* mean,
                                  double* var, double* kurtosis, int32_t* info, void* partials, size_t partials_bytes, void* stream);
int gpz_spatial_stats_plan(int64_t N, int64_t L, int32_t K, int32_t* row_chunk, int64_t* chunks, int64_t* partials_bytes);
int gpz_spatial_stats(const void* values, int64_t N, int64_t L, int32_t dtype, const int64_t* nbr, int32_t K, double* I, double* C,
                      double* mean, double* var, double* kurtosis, int32_t* info, void* partials, size_t partials_bytes, void* stream);

/* gpz_gene_morans_perm_sparse / gpz_morans_perm_rows with the statistic as an argument: stat 0 Moran's I, 1 Geary's C.  With
 * stat = 0 every output has the bits of those entries.  With stat = 1: value = the C of gpz_gene_spatial_stats_sparse, bit for
 * bit (the rows entry: the same expansion over all N spots); sims (D, P), may be NULL, C_pi -- under a relabelling only
 * Q_in,pi = sum_{i stored} indeg_pi(i) x_i^2 and C_s,pi change; n_ge / n_le the permutations with C_pi >= C and C_pi <= C,
 * decided on Q_in - 2 C_s in fp64, exact for integer-valued data below 2^53 (n_le counts towards positive autocorrelation);
 * sim_mean, sim_m2 of C_pi.  Everything else -- the arguments, info (1 a bad entry of nbr, 2 a row of perms that is no
 * permutation), line_mode, perm_batch, the plan query, reproducibility, independence of perm_batch and line_mode, an identity
 * row of perms giving the observed bits -- is as described there. */
int gpz_gene_autocorr_perm_sparse_plan(int64_t N, int64_t D, int64_t nnz, int32_t K, int64_t P, int32_t stat, int32_t perm_batch_wanted,
                                       int32_t line_mode_wanted, int32_t* perm_batch, int32_t* line_mode, int32_t* workgroups,
                                       int64_t* partials_bytes);
int gpz_gene_autocorr_perm_sparse(const int64_t* row_ptr, const int32_t* row_spot, const int32_t* row_perm, const float* col_val,
                                  const int64_t* nbr, const int32_t* perms, int64_t N, int64_t D, int64_t nnz, int32_t K, int64_t P,
                                  int32_t stat, int32_t perm_batch, int32_t line_mode, double* value, double* sims, int32_t* n_ge,
                                  int32_t* n_le, double* sim_mean, double* sim_m2, int32_t* info, void* partials, size_t partials_bytes,
                                  void* stream);
int gpz_autocorr_perm_rows_plan(int64_t N, int64_t D, int32_t K, int64_t P, int32_t stat, int32_t perm_batch_wanted,
                                int32_t line_mode_wanted, int32_t* perm_batch, int32_t* line_mode, int32_t* workgroups,
                                int64_t* partials_bytes);
int gpz_autocorr_perm_rows(const float* values, const int64_t* nbr, const int32_t* perms, int64_t N, int64_t D, int32_t K, int64_t P,
                           int32_t stat, int32_t perm_batch, int32_t line_mode, double* value, double* sims, int32_t* n_ge,
                           int32_t* n_le, double* sim_mean, double* sim_m2, int32_t* info, void* partials, size_t partials_bytes,
                           void* stream);

/* Residuals of counts under the predictive mean rate of a fitted count model, and Moran's I of every gene's residuals
 * (csrc/residual.hip).  With m = exp(mean + scale^2 / 2) (lognormal_mean != 0; exp(mean) otherwise) the rate is
 * mu[d,n] = V[n] sum_l W[d,l] m[l,n]; mean, scale (Lt, B), W (D, Lt), V (B,), theta (D,) (family 1; may be NULL for family 0).
 *   kind 0, Pearson:   r = (y - mu) / sqrt(mu (1 + mu / theta)); family 0 (Poisson): (y - mu) / sqrt(mu)
 *   kind 1, deviance:  r = sign(y - mu) sqrt(max(d, 0)), d = 2 (y log(y / mu) - (y - mu)) (Poisson, 2 mu at y = 0) or
 *                      d = 2 [y log(y / mu) - (y + theta) log1p((y - mu) / (mu + theta))] (family 1, negative binomial), in the
 *                      cancellation-free forms of gpz_poisson_deviance / gpz_nb_deviance
 * genes: int32 (G,) indices into [0, D), in any order and with repeats, or NULL for all genes (then G = D); an index outside
 * [0, D) gives a column of zeros.  Counts: y (D, B) dense, read once; or the by-gene arrays of a WHOLE data set stored as its
 * non-zeros (row_ptr, row_spot, row_perm, col_val as in gpz_gene_deviance_sparse; B = its N spots).  The sparse entries fill
 * every element with the zero-count residual (no counts are read) and then overwrite the stored entries, forming mu again at
 * each one in the dense pass's arithmetic: they give the bits of the dense entries on the densified counts.
 *   gpz_count_residuals*    out (B, G) fp32, spot-major: out[n * G + g] is the residual of listed gene g at spot n.
 *   gpz_residual_morans_i*  per listed gene, fp64 (G,): I = sum_n z_n (1 / K) sum_k z_nbr[n,k] / sum_n z_n^2 with
 *                           z = r - mean(r) (what gpz_morans_i gives for the column), res_mean = mean(r) and
 *                           res_var = sum_n z_n^2 / B.  nbr int64 (B, K), distinct neighbours; an entry outside [0, B) or
 *                           naming its own row is skipped and sets info[0] (device int32) to 1.  The genes are taken in
 *                           slabs of slab_genes columns of fp32 residuals, spot-major, inside `partials`; slab_genes = 0 takes
 *                           the plan's choice, the largest multiple of 64 with B * slab_genes * 4 bytes <= 256 MiB (at least
 *                           64, at most G rounded up to 64 and 2^20); a positive multiple of 64 overrides it.
 * Nothing of D x B or nnz elements is allocated.  fp32 element-wise work; every sum is fp64 in a fixed order, with no
 * atomics: two calls agree bit for bit.  gpz_residual_morans_i_plan (host-only; any out pointer may be NULL; D = the number
 * of scored genes) reports slab_genes, n_slabs, the tile shape and partials_bytes for the Moran entries; the residual
 * entries need no more than the partials of the plan with slab_genes_wanted = 64.  `partials` need not be cleared.
 * Limits, refused with -1 and the reason in gpz_last_error before any launch: 1 <= K <= 32, K < B < 2^31 (B < 2^27 with
 * stored counts), D, G, nnz < 2^31, 1 <= Lt <= 64, partials 16-byte aligned and large enough, family and kind 0 or 1. */
int gpz_residual_morans_i_plan(int64_t B, int64_t D, int32_t Lt, int64_t nnz, int64_t slab_genes_wanted, int64_t* slab_genes,
                               int64_t* n_slabs, int32_t* spots_per_tile, int32_t* genes_per_block, int32_t* spot_slices,
                               int32_t* gene_chunk, int32_t* factors_padded, int64_t* partials_bytes);
int gpz_count_residuals(const float* mean, const float* scale, const float* W, const float* V, const float* theta, const float* y,
                        const int32_t* genes, int64_t B, int64_t D, int64_t G, int32_t Lt, int32_t family, int32_t kind,
                        int32_t lognormal_mean, float* out, void* partials, size_t partials_bytes, void* stream);
int gpz_count_residuals_sparse(const float* mean, const float* scale, const float* W, const float* V, const float* theta,
                               const int64_t* row_ptr, const int32_t* row_spot, const int32_t* row_perm, const float* col_val,
                               const int32_t* genes, int64_t B, int64_t D, int64_t nnz, int64_t G, int32_t Lt, int32_t family,
                               int32_t kind, int32_t lognormal_mean, float* out, void* partials, size_t partials_bytes,
                               void* stream);
int gpz_residual_morans_i(const float* mean, const float* scale, const float* W, const float* V, const float* theta,
                          const float* y, const int32_t* genes, const int64_t* nbr, int64_t B, int64_t D, int64_t G, int32_t Lt,
                          int32_t K, int32_t family, int32_t kind, int32_t lognormal_mean, int64_t slab_genes, double* I,
                          double* res_mean, double* res_var, int32_t* info, void* partials, size_t partials_bytes, void* stream);
int gpz_residual_morans_i_sparse(const float* mean, const float* scale, const float* W, const float* V, const float* theta,
                                 const int64_t* row_ptr, const int32_t* row_spot, const int32_t* row_perm, const float* col_val,
                                 const int32_t* genes, const int64_t* nbr, int64_t B, int64_t D, int64_t nnz, int64_t G,
                                 int32_t Lt, int32_t K, int32_t family, int32_t kind, int32_t lognormal_mean, int64_t slab_genes,
                                 double* I, double* res_mean, double* res_var, int32_t* info, void* partials,
                                 size_t partials_bytes, void* stream);

/* Geary's C and the permutation null of the residuals (csrc/residual.hip; the column passes of csrc/spatial_stats.hip).  The
 * model arguments, the counts, genes, nbr, slab_genes and the slabs are those of gpz_residual_morans_i[_sparse]; the sparse
 * forms fill the slab exactly as there.
 *   gpz_residual_spatial_stats*   per listed gene, fp64 (G,): I, res_mean and res_var with gpz_residual_morans_i's bits; C,
 *                                 Geary's C of the residuals, (B - 1) sum_n sum_k (z_n - z_nbr[n,k])^2 / (2 B K sum_n z_n^2);
 *                                 kurtosis = m4 / m2^2 of the residuals, what the randomisation variances depend on.
 *   gpz_residual_autocorr_perm*   stat 0 Moran's I, 1 Geary's C.  value (G,): the observed statistic, the stats entry's bits.
 *                                 perms int32 (P, B): row p relabels the spots, r^pi[n] = r[pi[n]]; the slab is scored over
 *                                 the relabelled table T_pi[pi[i], m] = pi[nbr[i, m]] instead.  Per slab: the residual pass
 *                                 once, the wide column pass once, then every batch of perm_batch permutations (0: the
 *                                 plan's choice; at most 32), each batch one launch per (256-row chunk, 64-column tile)
 *                                 that reads a row of the slab once and gathers whole rows of the tile.  n_ge / n_le int32
 *                                 (G,): the permutations whose statistic is >= / <= the observed one, decided on the fp64
 *                                 numerators sum z lag / K (Moran) and sum (z_n - z_j)^2 (Geary) -- the denominator is
 *                                 common; residuals are real-valued, so a mathematical tie may fall either way in the last
 *                                 bit.  sim_mean, sim_m2 (G,): the mean of the simulated values and the sum of their squared
 *                                 deviations (Welford, in permutation order).  sims (G, P) fp64, may be NULL.  res_mean,
 *                                 res_var, kurtosis as above.  A partial sum of a permutation is folded in the order of the
 *                                 observed statistic's, so an identity row of perms gives `value` bit for bit, and nothing
 *                                 depends on perm_batch.  A gene with constant residuals has NaN values and counts nothing.
 * info[0] (device int32): 1 a bad entry of nbr (skipped), 2 a row of perms that is no permutation (the results are then
 * meaningless; nothing is read out of range).  No floating-point atomics; every sum fp64 in a fixed order.
 * gpz_residual_autocorr_perm_plan (host-only; any out pointer may be NULL; D = the number of scored genes) reports slab_genes,
 * n_slabs, perm_batch as resolved (a batch's tables, 4 B K bytes per permutation, stay within 256 MiB), the batches per slab
 * and partials_bytes: the slab, the factors, 40 bytes per (256-row chunk, slab column), and per permutation of a batch
 * 4 B (K + 1) bytes of tables plus 8 bytes per (chunk, slab column).  P = 0 asks for the scratch of the stats entries:
 * no tables and no permutations' partial sums, perm_batch = batches = 0.  Limits as for gpz_residual_morans_i, and P >= 1
 * for the permutation entries (P >= 0 for the query), stat 0 or 1, 0 <= perm_batch <= 32; refused with -1 and the reason
 * in gpz_last_error before any launch. */
int gpz_residual_autocorr_perm_plan(int64_t B, int64_t D, int32_t Lt, int32_t K, int64_t P, int64_t nnz, int64_t slab_genes_wanted,
                                    int32_t perm_batch_wanted, int64_t* slab_genes, int64_t* n_slabs, int32_t* perm_batch,
                                    int64_t* batches, int64_t* partials_bytes);
int gpz_residual_spatial_stats(const float* mean, const float* scale, const float* W, const float* V, const float* theta,
                               const float* y, const int32_t* genes, const int64_t* nbr, int64_t B, int64_t D, int64_t G, int32_t Lt,
                               int32_t K, int32_t family, int32_t kind, int32_t lognormal_mean, int64_t slab_genes, double* I,
                               double* C, double* res_mean, double* res_var, double* kurtosis, int32_t* info, void* partials,
                               size_t partials_bytes, void* stream);
int gpz_residual_spatial_stats_sparse(const float* mean, const float* scale, const float* W, const float* V, const float* theta,
                                      const int64_t* row_ptr, const int32_t* row_spot, const int32_t* row_perm, const float* col_val,
                                      const int32_t* genes, const int64_t* nbr, int64_t B, int64_t D, int64_t nnz, int64_t G,
                                      int32_t Lt, int32_t K, int32_t family, int32_t kind, int32_t lognormal_mean, int64_t slab_genes,
                                      double* I, double* C, double* res_mean, double* res_var, double* kurtosis, int32_t* info,
                                      void* partials, size_t partials_bytes, void* stream);
int gpz_residual_autocorr_perm(const float* mean, const float* scale, const float* W, const float* V, const float* theta,
                               const float* y, const int32_t* genes, const int64_t* nbr, const int32_t* perms, int64_t B, int64_t D,
                               int64_t G, int32_t Lt, int32_t K, int32_t family, int32_t kind, int32_t lognormal_mean,
                               int64_t slab_genes, int64_t P, int32_t stat, int32_t perm_batch, double* value, int32_t* n_ge,
                               int32_t* n_le, double* sim_mean, double* sim_m2, double* sims, double* res_mean, double* res_var,
                               double* kurtosis, int32_t* info, void* partials, size_t partials_bytes, void* stream);
int gpz_residual_autocorr_perm_sparse(const float* mean, const float* scale, const float* W, const float* V, const float* theta,
                                      const int64_t* row_ptr, const int32_t* row_spot, const int32_t* row_perm, const float* col_val,
                                      const int32_t* genes, const int64_t* nbr, const int32_t* perms, int64_t B, int64_t D,
                                      int64_t nnz, int64_t G, int32_t Lt, int32_t K, int32_t family, int32_t kind,
                                      int32_t lognormal_mean, int64_t slab_genes, int64_t P, int32_t stat, int32_t perm_batch,
                                      double* value, int32_t* n_ge, int32_t* n_le, double* sim_mean, double* sim_m2, double* sims,
                                      double* res_mean, double* res_var, double* kurtosis, int32_t* info, void* partials,
                                      size_t partials_bytes, void* stream);

/* Residuals of real-valued expression under a fitted Gaussian factor model, and the spatial autocorrelation of every gene's
 * residuals (csrc/residual.hip with csrc/residual_gaussian.h: the plan, the slabs and the driver of the count entries above).
 * mean, scale (Lt, B) are q(F); W (D, Lt) real; b (D,) the intercept; noise_sd (D,) positive.  With
 *   yhat[d,n] = b[d] + sum_l W[d,l] mean[l,n]   and   v[d,n] = noise_sd[d]^2 + sum_l W[d,l]^2 scale[l,n]^2
 * kind 0 is the Pearson residual (y - yhat) / noise_sd[d] (for a Gaussian also the deviance residual), kind 1 the response
 * residual y - yhat, kind 2 the predictive residual (y - yhat) / sqrt(v).  I and C do not change under a per-gene affine map,
 * so kinds 0 and 1 give the same I and C up to fp32 rounding; kind 2 differs spot by spot.  y (D, B) fp32 dense; the sparse
 * forms take the stored entries of the WHOLE data set in the by-gene order of gpz_poisson_nsf_sparse (N = B) and the fp64
 * offset (D,): y[d,n] = (float)((double)value - offset[d]), (float)(-offset[d]) where nothing is stored, and give the dense
 * entry's bits on that array.  genes, nbr, slab_genes, the outputs, perms, stat, perm_batch and info are those of
 * gpz_count_residuals, gpz_residual_spatial_stats and gpz_residual_autocorr_perm; the Gaussian entries always take the wide
 * column pass.  No floating-point atomics, every sum fp64 in a fixed order: two calls agree bit for bit.
 * gpz_gaussian_residual_plan (host-only; any out pointer may be NULL; D = the number of scored genes) reports what
 * gpz_residual_autocorr_perm_plan reports, with the residual pass's spot_slices and factors_padded; K = 0 (with P = 0) asks
 * for the scratch of gpz_gaussian_residuals[_sparse], the factors alone.  Limits: 1 <= Lt <= 64, 1 <= K <= 32 < B,
 * B, D, G, nnz < 2^31, B < 2^27 with stored entries, kind 0..2; refused with -1 and the reason in gpz_last_error before any
 * launch.  noise_sd is trusted to be positive and finite. */
int gpz_gaussian_residual_plan(int64_t B, int64_t D, int32_t Lt, int32_t K, int64_t P, int64_t nnz, int64_t slab_genes_wanted,
                               int32_t perm_batch_wanted, int64_t* slab_genes, int64_t* n_slabs, int32_t* spot_slices,
                               int32_t* factors_padded, int32_t* perm_batch, int64_t* batches, int64_t* partials_bytes);
int gpz_gaussian_residuals(const float* mean, const float* scale, const float* W, const float* b, const float* noise_sd,
                           const float* y, const int32_t* genes, int64_t B, int64_t D, int64_t G, int32_t Lt, int32_t kind,
                           float* out, void* partials, size_t partials_bytes, void* stream);
int gpz_gaussian_residuals_sparse(const float* mean, const float* scale, const float* W, const float* b, const float* noise_sd,
                                  const double* offset, const int64_t* row_ptr, const int32_t* row_spot, const int32_t* row_perm,
                                  const float* col_val, const int32_t* genes, int64_t B, int64_t D, int64_t nnz, int64_t G,
                                  int32_t Lt, int32_t kind, float* out, void* partials, size_t partials_bytes, void* stream);
int gpz_gaussian_residual_stats(const float* mean, const float* scale, const float* W, const float* b, const float* noise_sd,
                                const float* y, const int32_t* genes, const int64_t* nbr, int64_t B, int64_t D, int64_t G,
                                int32_t Lt, int32_t K, int32_t kind, int64_t slab_genes, double* I, double* C, double* res_mean,
                                double* res_var, double* kurtosis, int32_t* info, void* partials, size_t partials_bytes,
                                void* stream);
int gpz_gaussian_residual_stats_sparse(const float* mean, const float* scale, const float* W, const float* b, const float* noise_sd,
                                       const double* offset, const int64_t* row_ptr, const int32_t* row_spot,
                                       const int32_t* row_perm, const float* col_val, const int32_t* genes, const int64_t* nbr,
                                       int64_t B, int64_t D, int64_t nnz, int64_t G, int32_t Lt, int32_t K, int32_t kind,
                                       int64_t slab_genes, double* I, double* C, double* res_mean, double* res_var,
                                       double* kurtosis, int32_t* info, void* partials, size_t partials_bytes, void* stream);
int gpz_gaussian_residual_perm(const float* mean, const float* scale, const float* W, const float* b, const float* noise_sd,
                               const float* y, const int32_t* genes, const int64_t* nbr, const int32_t* perms, int64_t B, int64_t D,
                               int64_t G, int32_t Lt, int32_t K, int32_t kind, int64_t slab_genes, int64_t P, int32_t stat,
                               int32_t perm_batch, double* value, int32_t* n_ge, int32_t* n_le, double* sim_mean, double* sim_m2,
                               double* sims, double* res_mean, double* res_var, double* kurtosis, int32_t* info, void* partials,
                               size_t partials_bytes, void* stream);
int gpz_gaussian_residual_perm_sparse(const float* mean, const float* scale, const float* W, const float* b, const float* noise_sd,
                                      const double* offset, const int64_t* row_ptr, const int32_t* row_spot, const int32_t* row_perm,
                                      const float* col_val, const int32_t* genes, const int64_t* nbr, const int32_t* perms,
                                      int64_t B, int64_t D, int64_t nnz, int64_t G, int32_t Lt, int32_t K, int32_t kind,
                                      int64_t slab_genes, int64_t P, int32_t stat, int32_t perm_batch, double* value, int32_t* n_ge,
                                      int32_t* n_le, double* sim_mean, double* sim_m2, double* sims, double* res_mean,
                                      double* res_var, double* kurtosis, int32_t* info, void* partials, size_t partials_bytes,
                                      void* stream);

/* gpz_poisson_nsf for counts stored as their non-zeros (csrc/poisson_sparse.hip).  The sum of the rates factorises
 * (sum_{d,n} rate = sum_n V[n] sum_l c[l] expF[e,l,n], c[l] = sum_d W[d,l]) and y log(rate) is non-zero only where y is, so
 * loglik and the four gradients are exact sums over the non-zeros plus O(E Lt B + D Lt) dense terms: the same numbers as
 * gpz_poisson_nsf on the dense array, for nnz E Lt work.  No array of D x B or D x N elements exists, workspace included.
 * Counts of the WHOLE data set (D genes x N spots, nnz stored values) in two orders:
 *   by spot: col_ptr int64 (N + 1), col_gene int32 (nnz), col_val fp32 (nnz) -- spot n owns [col_ptr[n], col_ptr[n + 1]);
 *   by gene: row_ptr int64 (D + 1), row_spot int32 (nnz), row_perm int32 (nnz) = position of the same non-zero in the
 *            by-spot order (its value is col_val[row_perm[p]]).
 * Stored zeros contribute nothing (0 log(.) is never formed).  The arrays are trusted: indices in range, the two orders
 * consistent (gpzoo_amd.likelihoods.SparseCounts builds and checks them).
 * Batch: idx int32 (B,) = the global spot of each batch column, DISTINCT spots, and pos int32 (N,) = its inverse, -1 outside
 * the batch.  Both NULL: B == N and the identity.  mean, scale (Lt, B), eps (E, Lt, B), V (B,) are the batch's; W (D, Lt).
 * Outputs as gpz_poisson_nsf: loglik[2] fp64, dmean, dscale (Lt, B), dW (D, Lt), dV (B,), the mean over E applied.
 * 1 <= Lt <= 64; any E >= 1 (the kernels loop over the samples); N, D, nnz < 2^31.  W and ws must be 16-byte aligned.
 * Argument errors (null pointers, extents, Lt, a small workspace, alignment) return -1 before any launch.
 * No floating-point atomics, no workgroup waits on another, every sum in a fixed order: two calls agree bit for bit.
 * gpz_poisson_nsf_sparse_plan (host only, no device needed): gene_chunk = non-zeros of one gene row per wave of the gene
 * pass (512; a longer row is cut into chunks whose partial sums are added in chunk order), spot_chunk = the same for a
 * spot's column (0: columns are not split), n_gene_chunks = length of the gene pass's work list (D + nnz / gene_chunk, an
 * upper bound of the chunks in use), samples_per_group = samples the spot pass holds on chip at a time (E when they all
 * fit), factors_padded = Lt rounded up to the kernel instance.  Any out pointer may be NULL.
 * The workspace query returns 0 for refused arguments. */
int gpz_poisson_nsf_sparse_plan(int64_t N, int64_t B, int64_t D, int32_t Lt, int32_t E, int64_t nnz, int32_t* gene_chunk,
                                int32_t* spot_chunk, int64_t* n_gene_chunks, int32_t* samples_per_group,
                                int32_t* factors_padded);
size_t gpz_poisson_nsf_sparse_workspace_bytes(int64_t N, int64_t B, int64_t D, int64_t nnz, int32_t Lt, int32_t E);
int gpz_poisson_nsf_sparse(const float* mean, const float* scale, const float* eps, const float* W, const float* V,
                           const int64_t* col_ptr, const int32_t* col_gene, const float* col_val, const int64_t* row_ptr,
                           const int32_t* row_spot, const int32_t* row_perm, const int32_t* idx, const int32_t* pos,
                           int64_t N, int64_t B, int64_t D, int64_t nnz, int32_t Lt, int32_t E, int32_t with_lgamma,
                           double* loglik, float* dmean, float* dscale, float* dW, float* dV, void* ws, size_t ws_bytes,
                           void* stream);

/* gpz_nb_nsf for counts stored as their non-zeros (csrc/nb_sparse.hip): the six arrays, idx / pos and the batch convention
 * of gpz_poisson_nsf_sparse, with theta (D,) and dtheta (D,) as in gpz_nb_nsf.  With x = mu / theta the log-density is
 *   { -theta log1p(x) }  +  { y log(mu / (mu + theta)) + lgamma(y + theta) - lgamma(theta) - lgamma(y + 1) }:
 * the first brace needs no counts and runs over every (e, d, n) of the batch on the MFMA passes of gpz_nb_nsf without
 * their y operand (two transcendentals per element, log1p compensated); the second brace, and every gradient term with
 * a factor y, is zero where y is and is summed over the stored values of the batch -- one wave per batch spot (value, dV,
 * dmean, dscale) and one per 512-entry chunk of a gene row (dW, dtheta; the terms of y and theta alone in fp64, by
 * gpz_nb_nsf's recurrences for integer counts below 16 and lgamma / the digamma series otherwise).  A finishing kernel
 * adds the two parts in a fixed order.  Outputs as gpz_nb_nsf on the batch's dense counts: loglik[2], dmean, dscale
 * (Lt, B), dW (D, Lt), dV (B,), dtheta (D,), the mean over E applied.  A stored zero contributes exactly 0.
 * Nothing of D x B elements is read, written or allocated; the only workspace arrays whose length depends on nnz are per
 * chunk of the gene pass (D + nnz / gene_chunk entries).  No floating-point atomics, no workgroup waits on another:
 * two calls agree bit for bit.
 * 1 <= Lt <= 64, 1 <= E <= 32 per call, E Lt B < 2^29; N, D, nnz < 2^31.  mean, scale, eps, W, V, theta, the outputs and ws
 * must be 16-byte aligned.  Argument errors (null pointers, extents, Lt, E, a small workspace, alignment) return -1 before
 * any launch and name the entry in gpz_last_error; the workspace query then returns 0.
 * gpz_nb_nsf_sparse_plan (host only, no device needed; any out pointer may be NULL): gene_chunk = non-zeros of one gene
 * row per wave of the gene pass, n_gene_chunks = length of its work list (D + nnz / gene_chunk), factors_padded and
 * zero_factors_padded = Lt rounded up to the kernel instance of the non-zero passes and of the zero passes, gene_slices and
 * spot_slices = partial slabs of the zero part's spot pass and gene pass, samples_per_group and zero_samples_per_group =
 * samples held on chip at a time by the non-zero spot pass and by the zero gene pass. */
int gpz_nb_nsf_sparse_plan(int64_t N, int64_t B, int64_t D, int32_t Lt, int32_t E, int64_t nnz, int32_t* gene_chunk,
                           int64_t* n_gene_chunks, int32_t* factors_padded, int32_t* zero_factors_padded,
                           int32_t* gene_slices, int32_t* spot_slices, int32_t* samples_per_group,
                           int32_t* zero_samples_per_group);
size_t gpz_nb_nsf_sparse_workspace_bytes(int64_t N, int64_t B, int64_t D, int64_t nnz, int32_t Lt, int32_t E);
int gpz_nb_nsf_sparse(const float* mean, const float* scale, const float* eps, const float* W, const float* V,
                      const float* theta, const int64_t* col_ptr, const int32_t* col_gene, const float* col_val,
                      const int64_t* row_ptr, const int32_t* row_spot, const int32_t* row_perm, const int32_t* idx,
                      const int32_t* pos, int64_t N, int64_t B, int64_t D, int64_t nnz, int32_t Lt, int32_t E,
                      int32_t with_lgamma, double* loglik, float* dmean, float* dscale, float* dW, float* dV,
                      float* dtheta, void* ws, size_t ws_bytes, void* stream);

/* Poisson deviance under the predictive mean rate of a fitted factor model (csrc/deviance.hip), without materialising the
 * (D, N) rate.  fp32 inputs, fp64 outputs, no gradients.  mean, scale (Lt, N): q(F) moments of all factors at the N spots being
 * scored; W (D, Lt), V (N,): POSITIVE loadings / size factors; y (D, N) counts, read exactly once.
 *   m[l,n]   = exp(mean[l,n] + scale[l,n]^2 / 2)   (lognormal_mean != 0: E_q[exp F] exactly; 0: the plug-in exp(mean))
 *   mu[d,n]  = V[n] sum_l W[d,l] m[l,n]
 *   dev[d,n] = 2 (y log(y / mu) - y + mu), the log term exactly 0 at y = 0 (0 log 0 is never formed), so dev = 2 mu there
 * Outputs: per_gene (D,) = sum_n dev; per_spot (N,) = sum_d dev; null_per_gene (D,) = the deviance of the null model
 * mu0[d,n] = V[n] r_d, r_d = sum_n y[d,n] / sum_n V[n] (one constant rate per gene given the size factors), exactly 0 for a gene
 * without counts; scalars (4,) = {total, sum y, sum mu, null total}.  sum mu / sum y is the calibration of the size factors.
 * The null model's three per-gene sums (sum y, sum y log y, sum y log V) come from the same pass over y.
 * The rate tile is v_mfma_f32_16x16x4_f32 with the factors padded as gpz_poisson_nsf pads them; the unit deviance is formed
 * on the accumulator registers and reduced along both axes into partial slabs, which finishing kernels add in a fixed order
 * in fp64.  No floating-point atomics, no workgroup waits on another: two calls agree bit for bit.
 * 1 <= Lt <= 64; N, D < 2^31; N need not be a multiple of 4.  W and ws must be 16-byte aligned.  Argument errors (null
 * pointers, extents, Lt, a small workspace, alignment) return -1 before any launch; the workspace query then returns 0.
 * gpz_poisson_deviance_plan (host only, no device needed; any out pointer may be NULL): spots_per_tile x genes_per_tile = the
 * tile of one wave (64 x 16); genes_per_block = genes of one workgroup (64), gene_slices = ceil(D / genes_per_block) = the
 * number of per-spot partial slabs; spot_slices = number of per-gene partial slabs, each covering tiles_per_spot_slice
 * consecutive tiles; factors_padded = Lt rounded up to the kernel instance. */
int gpz_poisson_deviance_plan(int64_t N, int64_t D, int32_t Lt, int32_t* spots_per_tile, int32_t* genes_per_tile,
                              int32_t* genes_per_block, int32_t* gene_slices, int32_t* spot_slices,
                              int64_t* tiles_per_spot_slice, int32_t* factors_padded);
size_t gpz_poisson_deviance_workspace_bytes(int64_t N, int64_t D, int32_t Lt);
int gpz_poisson_deviance(const float* mean, const float* scale, const float* W, const float* V, const float* y, int64_t N,
                         int64_t D, int32_t Lt, int32_t lognormal_mean, double* per_gene, double* per_spot,
                         double* null_per_gene, double* scalars, void* ws, size_t ws_bytes, void* stream);

/* gpz_poisson_deviance for counts stored as their non-zeros: the six arrays, idx / pos and the batch convention of
 * gpz_poisson_nsf_sparse (both NULL: B == N and the identity); mean, scale (Lt, B), V (B,), W (D, Lt).  Where y = 0 the unit
 * deviance is 2 mu and sum mu factorises -- per gene sum_l W[d,l] a[l], a[l] = sum_n V[n] m[l,n]; per spot V[n] sum_l c[l] m[l,n],
 * c[l] = sum_d W[d,l] -- so every output is that dense term plus a sum over the stored values of 2 (y log(y / mu) - y):
 * O(nnz Lt + (D + B) Lt) work.  A gene or spot without stored values gets exactly the dense term; spots of the base matrix
 * outside the view contribute nothing, to the null model's sums either.  per_spot (B,) follows idx's order.
 * No array of D x B or D x N elements exists, workspace included, and the workspace holds nothing of nnz elements: the pass
 * by gene forms mu again at each non-zero (its chunk list has D + nnz / gene_chunk entries, which the query accounts for).
 * Same limits, alignment, error and reproducibility contract as gpz_poisson_deviance; nnz < 2^31.
 * gpz_poisson_deviance_sparse_plan (host only): gene_chunk = non-zeros of one gene row per wave (512; a longer row is cut
 * into chunks whose partial sums are added in chunk order), spot_chunk = the same for a spot's column (0: columns are not
 * split), n_gene_chunks = D + nnz / gene_chunk, factors_padded = Lt rounded up to the kernel instance. */
int gpz_poisson_deviance_sparse_plan(int64_t N, int64_t B, int64_t D, int32_t Lt, int64_t nnz, int32_t* gene_chunk,
                                     int32_t* spot_chunk, int64_t* n_gene_chunks, int32_t* factors_padded);
size_t gpz_poisson_deviance_sparse_workspace_bytes(int64_t N, int64_t B, int64_t D, int64_t nnz, int32_t Lt);
int gpz_poisson_deviance_sparse(const float* mean, const float* scale, const float* W, const float* V, const int64_t* col_ptr,
                                const int32_t* col_gene, const float* col_val, const int64_t* row_ptr,
                                const int32_t* row_spot, const int32_t* row_perm, const int32_t* idx, const int32_t* pos,
                                int64_t N, int64_t B, int64_t D, int64_t nnz, int32_t Lt, int32_t lognormal_mean,
                                double* per_gene, double* per_spot, double* null_per_gene, double* scalars, void* ws,
                                size_t ws_bytes, void* stream);

/* Held-out scoring under a negative-binomial likelihood with one inverse dispersion theta[d] > 0 per gene (torch's
 * NegativeBinomial(total_count = theta, logits = log mu - log theta)) and the predictive mean rate of gpz_poisson_deviance,
 * mu[d,n] = V[n] sum_l W[d,l] m[l,n]: the interface of gpz_poisson_deviance plus theta (D,).
 *   dev = 2 [ y log(y / mu) - (y + theta) log1p((y - mu) / (mu + theta)) ]        (the first term exactly 0 at y = 0)
 *   ll  = lgamma(y + theta) - lgamma(theta) - lgamma(y + 1) + y log(mu / (mu + theta)) - theta log1p(mu / theta)
 *   pll = y log mu - mu - lgamma(y + 1)                                            (the Poisson log density of the same mu)
 * per_gene, null_per_gene, loglik_per_gene, poisson_loglik_per_gene (D,), per_spot, loglik_per_spot (N,) and
 * scalars[6] = {total, sum y, sum mu, null total, loglik, poisson loglik}, all fp64.  The null model is mu0[d,n] = V[n] r_d
 * with the Poisson null's rate r_d = sum_n y / sum_n V and the gene's own theta (the maximum-likelihood rate when V is
 * constant, a convention otherwise); null_per_gene is exactly 0 for a gene without counts.
 * fp32 element-wise work (a compensated log1p), the lgamma terms and every sum in fp64 in a fixed order, no atomics: two calls
 * agree bit for bit.  y is read twice (sum_n y must be known before the null deviance can be evaluated); the (D, N) rate never
 * exists in memory and the workspace holds nothing of D x N elements.  Limits, alignment and the error contract are those of
 * gpz_poisson_deviance; a null theta is rejected with a message of its own.  gpz_nb_deviance_plan answers like
 * gpz_poisson_deviance_plan. */
int gpz_nb_deviance_plan(int64_t N, int64_t D, int32_t Lt, int32_t* spots_per_tile, int32_t* genes_per_tile,
                         int32_t* genes_per_block, int32_t* gene_slices, int32_t* spot_slices, int64_t* tiles_per_spot_slice,
                         int32_t* factors_padded);
size_t gpz_nb_deviance_workspace_bytes(int64_t N, int64_t D, int32_t Lt);
int gpz_nb_deviance(const float* mean, const float* scale, const float* W, const float* V, const float* theta, const float* y,
                    int64_t N, int64_t D, int32_t Lt, int32_t lognormal_mean, double* per_gene, double* per_spot,
                    double* null_per_gene, double* loglik_per_gene, double* loglik_per_spot, double* poisson_loglik_per_gene,
                    double* scalars, void* ws, size_t ws_bytes, void* stream);

/* gpz_nb_deviance for counts stored as their non-zeros; the argument layout of gpz_poisson_deviance_sparse plus theta.  With
 * z(mu) = theta log1p(mu / theta) every output is a zero part over ALL (d, n) of the batch -- 2 z for the deviance, -z for the
 * log density, -mu for the Poisson log density, from one dense pass that reads no counts -- plus a sum over the stored values:
 *   dev: 2 [ y log(y (mu + theta) / (mu (y + theta))) - theta log1p(y / theta) ]
 *   ll:  y log(mu / (mu + theta)) + lgamma(y + theta) - lgamma(theta) - lgamma(y + 1);      pll: y log mu - lgamma(y + 1)
 * The null model's rate comes first from a pass over the gene rows' stored entries.  The workspace holds nothing of D x B or
 * nnz elements.  Same contract as gpz_poisson_deviance_sparse; gpz_nb_deviance_sparse_plan answers like its plan query. */
int gpz_nb_deviance_sparse_plan(int64_t N, int64_t B, int64_t D, int32_t Lt, int64_t nnz, int32_t* gene_chunk,
                                int32_t* spot_chunk, int64_t* n_gene_chunks, int32_t* factors_padded);
size_t gpz_nb_deviance_sparse_workspace_bytes(int64_t N, int64_t B, int64_t D, int64_t nnz, int32_t Lt);
int gpz_nb_deviance_sparse(const float* mean, const float* scale, const float* W, const float* V, const float* theta,
                           const int64_t* col_ptr, const int32_t* col_gene, const float* col_val, const int64_t* row_ptr,
                           const int32_t* row_spot, const int32_t* row_perm, const int32_t* idx, const int32_t* pos, int64_t N,
                           int64_t B, int64_t D, int64_t nnz, int32_t Lt, int32_t lognormal_mean, double* per_gene,
                           double* per_spot, double* null_per_gene, double* loglik_per_gene, double* loglik_per_spot,
                           double* poisson_loglik_per_gene, double* scalars, void* ws, size_t ws_bytes, void* stream);

/* K nearest rows of Z for every row of X, ascending by (Euclidean distance, index): the neighbour
 * bookkeeping of VNNGP, argsort(cdist(X, Z))[:, :K] (gp.py:31, 64).  idx (N,K) int64.  K <= 32. */
int gpz_knn(const void* X, int64_t N, const void* Z, int64_t M, int32_t d, int32_t K, int32_t dtype,
            int64_t* idx, void* stream);

/* VNNGP.forward (gp.py:21-122).  Accepted kernel kinds: GPZ_KERNEL_RBF, GPZ_KERNEL_MATERN32, GPZ_KERNEL_MATERN12 and
 * GPZ_KERNEL_MATERN52 (the reference asks return_distance of its kernel and nothing else: its RBF family has it, a
 * Matern kernel gets it in one line); GPZ_KERNEL_MGGP_RBF is refused (non-zero return, gpz_last_error names the kind)
 * -- the reference has no multi-group VNNGP.  Uses the problem's X, Z, kernel, mu, Lu_raw, jitter, var_clamp_min (the reference clamps at 5e-2) and
 * writes mean, scale (L,N), optionally Lu and chol, and info.  idx: (N,K) neighbour lists from
 * gpz_knn, or NULL to compute them here. */
size_t gpz_vnngp_workspace_bytes(const gpz_svgp_problem* p, int32_t K);
/* Hand-off from gpz_vnngp_forward to the gpz_vnngp_backward of the same call: with `factor_cache` pointing at
 * gpz_vnngp_state_bytes(p) bytes (caller owned) the forward leaves Kzz + jitter I, its factor, Lu, S = Lu Lu^T and -- when
 * it evaluates `kl` -- L^{-1}, L^{-1} Lu, L^{-1} mu there; a backward pass given the same buffer with factor_cache_valid =
 * 1 (factor, Lu, S) | 4 (the KL operands) reads them instead of forming them again.  The backward pass uses parts of the
 * buffer as scratch: it is valid for ONE backward.  NULL: every pass forms what it needs in its workspace. */
size_t gpz_vnngp_state_bytes(const gpz_svgp_problem* p);
int gpz_vnngp_forward(const gpz_svgp_problem* p, int32_t K, const int64_t* idx, void* ws,
                      size_t ws_bytes, void* stream);

/* Backward of VNNGP.forward as loss.backward() runs it through the reference's autograd graph
 * (utilities.py:485 over gp.py:21-122): given dLoss/dmean, dLoss/dscale (and, for the kernel
 * hyper-parameters, dLoss/dchol from KL(qU || pU)) writes grad_mu, grad_Lu_raw and, when
 * grad_theta / grad_Z are non-NULL, the gradients w.r.t. (sigma, lengthscale) per latent and Z.
 * Kernel kinds as gpz_vnngp_forward; dk/dz of a datum that coincides with its inducing point is 0 (the r -> 0 limit for
 * Matern-3/2 and -5/2, the convention of gpz_kgrad at the kink of Matern-1/2).
 * The neighbour table is a constant of the graph (argsort has no gradient).  `scale` of
 * gpz_svgp_grads is unused (the variance is recomputed); `g_kl` folds the gradient of the forward's
 * per-latent KL(qU || pU) (problem field `kl`) in, as in gpz_svgp_backward.  The K-sparse terms (the sums over the
 * points that name an inducing point) are formed in a fixed order over the inverted neighbour table -- no atomics on
 * values, bitwise reproducible.  A caller-supplied idx may repeat a neighbour inside a row (checked on the device; those
 * calls add lane after lane); its entries must lie in [0, M).  Limits of the backward pass beyond the forward's:
 * M <= 8192 (two fp64 rows of the padded order in 128 KB of LDS) and N * K < 2^31. */
size_t gpz_vnngp_backward_workspace_bytes(const gpz_svgp_problem* p, int32_t K);
int gpz_vnngp_backward(const gpz_svgp_problem* p, const gpz_svgp_grads* g, int32_t K,
                       const int64_t* idx, void* ws, size_t ws_bytes, void* stream);

/* Moments from a caller-supplied W (L,N,M): WSVGP.forward_precomputed, gp.py:308-322
 * (cov = clamp(sigma^2 - sum W^2, 0) + sum (W Lu)^2, mean = W mu).  sigma (L,), mu (L,M),
 * Lu_raw (L,M,M) -> mean, scale (L,N) and the constrained Lu (L,M,M, may be NULL). */
size_t gpz_wsvgp_precomputed_workspace_bytes(int64_t L, int64_t N, int64_t M, int32_t dtype);
int gpz_wsvgp_precomputed(const void* W, const void* sigma, const void* mu, const void* Lu_raw,
                          int64_t L, int64_t N, int64_t M, int32_t dtype, void* mean, void* scale,
                          void* Lu, void* ws, size_t ws_bytes, void* stream);

/* Backward of gpz_wsvgp_precomputed -- what loss.backward() sends through gp.py:308-322 to mu, Lu and the
 * kernel's sigma (W is the caller's constant): given dLoss/dmean, dLoss/dscale and the forward's scale (L,N)
 * writes grad_mu (L,M), grad_Lu_raw (L,M,M, zeros above the diagonal) and, if non-NULL, grad_sigma (L,) fp64. */
size_t gpz_wsvgp_precomputed_backward_workspace_bytes(int64_t L, int64_t N, int64_t M, int32_t dtype);
int gpz_wsvgp_precomputed_backward(const void* W, const void* sigma, const void* mu, const void* Lu_raw,
                                   int64_t L, int64_t N, int64_t M, int32_t dtype, const void* g_mean,
                                   const void* g_scale, const void* scale, void* grad_mu, void* grad_Lu_raw,
                                   double* grad_sigma, void* ws, size_t ws_bytes, void* stream);

/* Self-kNN graph of N points (X (N,d) of `dtype`, row-major): idx (N,K) int64, row i = the K points nearest to point i,
 * self excluded, ascending by (d^2, original index), where d^2 is sklearn's: the coordinates converted to fp64, each
 * (x_k - y_k)^2 rounded, the terms added in coordinate order.  Other points at distance 0 are ordinary neighbours.
 * Exact -- what squidpy's spatial_neighbors(coord_type="generic", n_neighs=K) builds through
 * NearestNeighbors.kneighbors() (dims_autocorr, utilities.py:149), except where an exact tie at the K-th distance is
 * broken by its KD-tree's visit order there.  1 <= d <= 4, 1 <= K <= 32, K < N < 2^31.
 * `order` (N,) int64 or NULL: the order in which the points are searched (a space-filling curve makes each group of 64
 * queries spatially compact, so most candidate tiles are skipped on their bounding boxes).  The graph does not depend on
 * it; an order that is not a permutation of [0, N) is detected on the device and the identity is used instead.  A
 * non-finite coordinate ranks its pairs as +inf (behind every finite one): every slot is still a valid index. */
size_t gpz_spatial_knn_workspace_bytes(int64_t N, int32_t d, int32_t K);
int gpz_spatial_knn(const void* X, int64_t N, int32_t d, int32_t K, int32_t dtype, const int64_t* order, int64_t* idx,
                    void* ws, size_t ws_bytes, void* stream);

/* Moran's I of every column of values (N,L) of `dtype`, row-major, over a K-neighbour graph nbr (N,K) int64 with
 * row-normalised weights 1/K -- squidpy's spatial_autocorr(mode="moran", transformation=True):
 *   z = v - mean(v),  I = sum_i z_i (1/K sum_{j in nbr(i)} z_j) / sum_i z_i^2   (N / S0 = 1),
 * I (L,) fp64; a constant column gives 0 / 0 = NaN (the mean is formed around the column's first value, so it is
 * exact for a constant column).  Every sum is taken in a fixed order: repeated calls agree bit for bit.  Each entry of
 * nbr is checked on the device: one outside [0, N) or equal to its row is not read, and info[0] (device int32) is set
 * to 1.  1 <= K < N < 2^31, 1 <= L <= 2^20. */
size_t gpz_morans_i_workspace_bytes(int64_t N, int64_t L, int32_t K);
int gpz_morans_i(const void* values, int64_t N, int64_t L, int32_t dtype, const int64_t* nbr, int32_t K, double* I,
                 int32_t* info, void* ws, size_t ws_bytes, void* stream);

/* KL-divergence NMF by multiplicative updates: X (N,D) >= 0, dense row-major, ~ W (N,L) . H (L,D), all of `dtype`.
 * One iteration is sklearn's _multiplicative_update_w followed by _multiplicative_update_h for beta_loss = 1, no
 * regularisation (EPS = the float32 epsilon in both precisions):
 *   P = W H, P[P < EPS] = EPS, Q = X / P;  W *= (Q H^T) / rowsum(H)             (a zero rowsum reads as EPS)
 *   P = W H with the new W, clamped, Q = X / P;  H *= (W^T Q) / colsum(W)[:, None]  (a zero colsum reads as 1)
 *   H[H < the float64 epsilon] = 0.
 * gpz_nmf_kl_update runs `iters` >= 1 iterations on W and H in place.  P and Q are never stored: per iteration X is read
 * twice and nothing of size N x D is written; the sum over N of the H update goes through per-slab partial sums in the
 * workspace.  No atomics, every sum in a fixed order: repeated calls on the same input agree bit for bit, and one call of
 * 2 k iterations equals two calls of k.
 * gpz_nmf_kl_divergence writes sklearn's _beta_divergence(X, W, H, 1, square_root=True) to out (device fp64):
 *   sqrt(2 max(0, sum_{X > EPS} X log(X / max(W H, EPS)) + colsum(W) . rowsum(H) - sum_{X > EPS} X)), summed in fp64.
 * X must be finite and non-negative (not checked here).  1 <= L <= 64, N, D >= 1, N, D < 2^31, N D < 2^40; anything
 * else is an argument error on the host, before any launch (the workspace query then returns 0). */
size_t gpz_nmf_kl_workspace_bytes(int64_t N, int64_t D, int64_t L, int32_t dtype);
int gpz_nmf_kl_update(const void* X, void* W, void* H, int64_t N, int64_t D, int64_t L, int32_t dtype, int64_t iters,
                      void* ws, size_t ws_bytes, void* stream);
int gpz_nmf_kl_divergence(const void* X, const void* W, const void* H, int64_t N, int64_t D, int64_t L, int32_t dtype,
                          double* out, void* ws, size_t ws_bytes, void* stream);

/* The same NMF for counts held as their non-zeros (gpzoo_amd.likelihoods.SparseCounts, the six arrays of
 * gpz_poisson_nsf_sparse): the counts are (D genes, N spots) and X[n,d] = counts[d,n], so the by-spot order lists the
 * non-zeros of a row of X (the W update reads it) and the by-gene order those of a column (the H update reads it).
 * Q = X / max(W H, EPS) is zero wherever X is: both numerators are sums over the stored values, the denominators are
 * rowsum(H) and colsum(W), and the divergence is sum_{x > EPS} x log(x / max(p, EPS)) + colsum(W) . rowsum(H) - sum x.
 * One iteration has the semantics of gpz_nmf_kl_update (same clamps, same zero-sum rules, H < float64 epsilon -> 0; a spot
 * or gene without non-zeros gets a zero numerator) for O(nnz L) work; nothing of N x D or of nnz elements is allocated.
 * W (N,L) and H (L,D) row-major of `dtype`, updated in place; col_val is fp32 whatever the dtype.  1 <= L <= 64 (padded to
 * the kernel instance 4 8 12 16 20 24 32 40 48 64 with zeros), N, D >= 1, nnz >= 0 (the four per-non-zero arrays may be
 * NULL when nnz == 0), N, D, nnz < 2^31; ws 16-byte aligned.  Argument errors return -1 before any launch and the
 * workspace query then returns 0.  No floating-point atomics, no workgroup waits on another, every sum in a fixed order:
 * two calls agree bit for bit and one call of 2 k iterations equals two of k.
 * gpz_nmf_kl_sparse_plan (host only, no device needed): spot_chunk = non-zeros of a spot's row per wave of the W pass (0:
 * rows are not split), gene_chunk = the same for a gene's row in the H pass (a longer row is cut into chunks whose
 * partial sums are added in chunk order), n_gene_chunks = D + nnz / gene_chunk, an upper bound of the chunks in use,
 * factors_padded = L rounded up to the kernel instance, colsum_rows = rows per block of the partial sums behind
 * colsum(W) and rowsum(H).  Any out pointer may be NULL. */
int gpz_nmf_kl_sparse_plan(int64_t N, int64_t D, int64_t nnz, int32_t L, int32_t dtype, int32_t* spot_chunk,
                           int32_t* gene_chunk, int64_t* n_gene_chunks, int32_t* factors_padded, int32_t* colsum_rows);
size_t gpz_nmf_kl_sparse_workspace_bytes(int64_t N, int64_t D, int64_t nnz, int32_t L, int32_t dtype);
int gpz_nmf_kl_sparse_update(const int64_t* col_ptr, const int32_t* col_gene, const float* col_val, const int64_t* row_ptr,
                             const int32_t* row_spot, const int32_t* row_perm, void* W, void* H, int64_t N, int64_t D,
                             int64_t nnz, int32_t L, int32_t dtype, int64_t iters, void* ws, size_t ws_bytes, void* stream);
int gpz_nmf_kl_sparse_divergence(const int64_t* col_ptr, const int32_t* col_gene, const float* col_val,
                                 const int64_t* row_ptr, const int32_t* row_spot, const int32_t* row_perm, const void* W,
                                 const void* H, int64_t N, int64_t D, int64_t nnz, int32_t L, int32_t dtype, double* out,
                                 void* ws, size_t ws_bytes, void* stream);

/* Products of the same counts with a thin fp64 matrix, for the subspace iteration behind the NNDSVD start:
 * transpose = 0: out (N,k) = X Q, Q (D,k);  transpose = 1: out (D,k) = X^T Q, Q (N,k);  row-major, 1 <= k <= 128.
 * One wave per spot, or per chunk of a gene's row with the chunk partials added in chunk order; the stored values of a row
 * are added in their stored order: bitwise repeatable.  Argument errors as above. */
size_t gpz_counts_matmul_workspace_bytes(int64_t N, int64_t D, int64_t nnz, int32_t k, int32_t transpose);
int gpz_counts_matmul(const int64_t* col_ptr, const int32_t* col_gene, const float* col_val, const int64_t* row_ptr,
                      const int32_t* row_spot, const int32_t* row_perm, const double* Q, double* out, int64_t N, int64_t D,
                      int64_t nnz, int32_t k, int32_t transpose, void* ws, size_t ws_bytes, void* stream);

/* Exact K-nearest mean: for each of M query points Z (M,d) the mean of F (N,L) over the K points of X (N,d) nearest to it
 * -- sklearn's KNeighborsRegressor(n_neighbors=K).fit(X, F).predict(Z) with uniform weights (smooth_spatial_factors,
 * utilities.py:66-67).  X and Z share `dtype`, F has `f_dtype` (fp32 or fp64 each), all row-major.  d^2 is sklearn's: the
 * coordinates converted to fp64, each (x_k - z_k)^2 rounded, the terms added in coordinate order; a NaN d^2 ranks as +inf.
 * The K smallest keys (d^2, index) are selected -- exact ties go to the lower index, which is sklearn's set wherever no
 * exact tie falls on the K-th place -- by a radix select on the bit pattern of d^2, recomputed in every pass: nothing of
 * size M x N is stored and nothing is sorted.
 *   U (M,L) fp64: U[m] = (sum of F[n] over the selected n) / K, fp64 accumulators, the spots dealt to threads and the
 *   partial sums combined in a fixed order, no floating-point atomics: repeated calls agree bit for bit.
 *   idx (M,K) int64 or NULL: the selected points of each query in ASCENDING INDEX order (not by distance).
 * 1 <= d <= 4, 1 <= K <= N < 2^31, 1 <= M < 2^31, 1 <= L <= 256; anything else is an argument error on the host, before
 * any launch (the workspace query then returns 0).  The workspace holds the fp64 coordinates: (N + M) d doubles. */
size_t gpz_knn_mean_workspace_bytes(int64_t N, int64_t M, int32_t d, int64_t K, int64_t L);
int gpz_knn_mean(const void* X, int64_t N, const void* Z, int64_t M, int32_t d, int32_t dtype, const void* F, int64_t L,
                 int32_t f_dtype, int64_t K, double* U, int64_t* idx, void* ws, size_t ws_bytes, void* stream);

/* k-means for the inducing points: Z = the centres of sklearn's KMeans(n_clusters=M, n_init=1, algorithm="lloyd") on the
 * spots X (N,d), fp32 or fp64 by `dtype`, row-major, dense, no sample weights.  Centres C (M,d) are fp64 throughout.
 * Shared arithmetic: d^2 is the kNN distance of gpz_knn_mean (coordinates as fp64, each (x_k - c_k)^2 rounded, added in
 * coordinate order; a NaN d^2 ranks as +inf); a point's label is the arg-min over (d^2, centre index): ties go to the
 * lower index.  No floating-point atomics; every sum is fp64 in an order fixed by the shapes: repeated calls agree bit for
 * bit.  No kernel waits on another workgroup.  1 <= d <= 4, 1 <= M <= N < 2^31; anything else is an argument error on the
 * host, before any launch (the workspace queries then return 0).  Each workspace holds the fp64 points and O(N + M) scratch
 * (plus 12 N bytes per centre split when N is small against the chip).
 *
 * gpz_kmeans_lloyd runs up to `iters` (1..2^20) further iterations of sklearn's lloyd_iter + the stopping rules of
 * _kmeans_single_lloyd, C in place.  One iteration: labels w.r.t. the current centres (labels (N,) int32 in/out: on entry
 * the previous iteration's labels, -1 everywhere before the first); each new centre the fp64 mean of its members (lane j of
 * one wave per cluster sums the members among the points j mod 64 in ascending index, the lanes by a fixed tree); empty
 * clusters relocated as _relocate_empty_clusters_dense does -- skipped when max d^2 = 0, else the n_empty points with the
 * largest d^2 to their own old centre, ties to the lower index, taken in descending order by the empty clusters in
 * ascending index, each subtracted from the sum and count of the cluster it leaves (sklearn's set of points; its pairing
 * for more than one empty cluster is argpartition's, which is unspecified) --; a cluster left without a member stays at
 * its old centre; shift = sum ||c_new - c_old||^2.  Stop reason 1 when no label changed, else 2 when shift <= tol_abs
 * (the caller's tol * mean(var(X, axis=0))).  `state` is a caller-owned DEVICE record, zeroed before the first call; every
 * launch of an iteration returns at once when state->stop is set, so a caller enqueues a block of iterations and reads the
 * record once per block.  After a stop other than 1 (or none) the labels are one iteration behind the centres:
 * gpz_kmeans_assign gives the final ones.  Lloyd from a given start is sklearn-exact (labels, n_iter_) wherever no point
 * lies within rounding of two centres.
 *
 * gpz_kmeans_assign: keep_labels = 0 writes labels[n] = arg-min (the final labelling step, or "which inducing point owns
 * this spot"); keep_labels = 1 takes labels as given (one outside [0, M) has d^2 = +inf).  d2_out (N,) fp64 or NULL: d^2 of
 * each point to its label's centre.  inertia_out (device fp64) or NULL: their sum, 256 points per block total and the block
 * totals in block order.
 *
 * gpz_kmeans_seed: greedy k-means++ (sklearn's _kmeans_plusplus) with the random stream passed in: u (M,T) fp64 on the
 * device, uniform in [0, 1), T (1..32; sklearn's 2 + floor(ln M)) trials per centre.  The first index is floor(u[0,0] N);
 * for c = 1..M-1 candidate t is the smallest i with cumsum(closest_d2)[i] >= u[c,t] pot, clipped to N - 1 (index 0 when
 * pot = 0), the cumulative sum in two levels (totals of blocks of 256 points, then inside the chosen block); the candidate
 * whose sum of min(closest_d2, d^2(candidate, .)) is smallest wins, ties to the lower t.  idx_out (M,) int64 the chosen
 * points, C_out (M,d) fp64 their coordinates.  The stream is defined here (numpy's default_rng in the Python wrapper), so a
 * seeded result differs from sklearn's for the same random_state.  M - 1 dependent steps of four short launches. */
typedef struct gpz_kmeans_state {
  int64_t iterations; /* iterations done over all calls */
  int64_t stop;       /* 0 = none, 1 = the labels repeated, 2 = shift <= tol_abs */
  double shift;       /* of the last iteration */
  int64_t relocated;  /* points given to empty clusters, over all iterations */
} gpz_kmeans_state;
size_t gpz_kmeans_seed_workspace_bytes(int64_t N, int32_t d, int64_t M, int32_t T);
int gpz_kmeans_seed(const void* X, int64_t N, int32_t d, int32_t dtype, int64_t M, int32_t T, const double* u,
                    int64_t* idx_out, double* C_out, void* ws, size_t ws_bytes, void* stream);
size_t gpz_kmeans_lloyd_workspace_bytes(int64_t N, int32_t d, int64_t M);
int gpz_kmeans_lloyd(const void* X, int64_t N, int32_t d, int32_t dtype, double* C, int64_t M, double tol_abs, int64_t iters,
                     int32_t* labels, gpz_kmeans_state* state, void* ws, size_t ws_bytes, void* stream);
size_t gpz_kmeans_assign_workspace_bytes(int64_t N, int32_t d, int64_t M);
int gpz_kmeans_assign(const void* X, int64_t N, int32_t d, int32_t dtype, const double* C, int64_t M, int32_t keep_labels,
                      int32_t* labels, double* d2_out, double* inertia_out, void* ws, size_t ws_bytes, void* stream);

/* Normal equations of the kernel least-squares projection of factors onto the inducing points -- what
 * Slideseqv2_estimate_lengthscales.ipynb (build_model_scracth: L1 = cholesky(add_jitter(Kzx @ Kxz, 1e-5)),
 * alpha = cholesky_solve(Kzx @ F, L1), mu = Kzz @ alpha) and NSF_Hybrid_benchmark.ipynb (torch.pinverse(Kzx @ Kxz)) form
 * from a materialised Kzx = kernel(Z, X):
 *   G[l] = K_zx K_xz + jitter I   (n_latent, M, M) fp64, full symmetric (the upper triangle is the mirrored lower one),
 *   b[l] = K_zx F[l]^T            (n_latent, R, M) fp64,        K_zx = k_l(Z, X),
 * in ONE pass over X: neither K_zx nor an N-sized piece of it is written to memory.  k: kinds GPZ_KERNEL_RBF, _MATERN32,
 * _MATERN12, _MATERN52 (anything else is refused); Z (M,d), X (N,d) and F (n_latent, R, N) of k->dtype, R right-hand sides
 * per latent (a scalar-parameter kernel passes n_latent = 1 and its L factor rows as R).  Limits, argument errors on the
 * host before any launch: 1 <= d <= 4, 1 <= R <= 64, 1 <= N < 2^31, 1 <= M <= 8192, n_latent <= 65535, jitter >= 0.
 * Arithmetic: k->dtype = GPZ_F32 generates the covariance entries in fp32 -- the bits gpz_kfill writes -- and multiplies
 * and adds them in fp32 (v_mfma_f32_16x16x4_f32) inside one N-split of at most 16 384 columns; GPZ_F64 does both in fp64
 * (v_mfma_f64_16x16x4_f64).  The splits' partial sums are added in ascending split order in fp64 in both cases.  No
 * floating-point atomics, no kernel waits on another workgroup (one plain grid and one reduction launch): two calls on
 * the same input agree bit for bit.
 * gpz_kernel_gram_plan (host only, no device needed): tile = rows and columns of an output tile (128), col_step = columns
 * of X one step of a workgroup covers (32 fp32, 16 fp64), n_splits and cols_per_split (a multiple of col_step, at least
 * 4 col_step; the last split may be shorter): n_splits = ceil(N / cols_per_split), chosen so that a split has at most
 * 16 384 columns and the launch at least 512 workgroups where N allows.  Any out pointer may be NULL.
 * Workspace: the splits' partial tiles only, n_splits x n_latent x (nt (nt + 1) / 2 x 128 x 128 + nt x RB x 128) values
 * of k->dtype, nt = ceil(M / 128), RB = 16 for R <= 16 else 64 (plus alignment): for a fixed number of splits it does not
 * depend on N, and from M = 1024 on it is smaller than n_splits x sizeof(G).  The query returns 0 for a refused shape. */
int gpz_kernel_gram_plan(int64_t N, int64_t M, int32_t n_latent, int32_t dtype, int32_t* tile, int32_t* col_step,
                         int32_t* n_splits, int64_t* cols_per_split);
size_t gpz_kernel_gram_workspace_bytes(int64_t N, int64_t M, int32_t n_latent, int32_t R, int32_t dtype);
int gpz_kernel_gram(const gpz_kernel_desc* k, const void* Z, int64_t M, const void* X, int64_t N, int32_t d, const void* F,
                    int32_t R, double jitter, double* G, double* b, void* ws, size_t ws_bytes, void* stream);

/* Multi-GPU: latent GPs shard across ranks with no data-path collective; the only exchange is
 * the sum of each rank's partial ELBO -- one ncclAllReduce(sum, fp64) over RCCL/xGMI.  The reference has no
 * distributed code to cite; this is the entry SURVEY §8b proposes.  One communicator per process
 * (rank <-> GPU): rank 0 calls gpz_comm_unique_id and hands the 128 bytes to every rank (file, socket, MPI,
 * torch's store, ...), each rank then calls gpz_comm_init with its HIP device current.  `comm` may equally be
 * an ncclComm_t the caller created itself.  gpz_allreduce_sum_f64 sums buf[0..n) in place over the ranks,
 * asynchronously on `stream`.  RCCL is bound at run time (dlopen): the rest of the library works without it. */
int gpz_comm_unique_id(void* id128_host);
int gpz_comm_init(void** comm_out, int32_t world, int32_t rank, const void* id128_host);
int gpz_allreduce_sum_f64(void* comm, double* buf, int64_t n, void* stream);
/* The latent-sharded Poisson NSF step (reference likelihoods.py:49-53, 74-97: rate = softplus(W) @ exp(F) mixes the
 * latents, SURVEY §8e "Caveat"): every rank gathers q(F)'s moments of all latents -- gpz_allgather, `bytes_per_rank`
 * bytes from each rank into recv[rank * bytes_per_rank ...), 2 L N_b s bytes in all against D N_b s for exchanging
 * partial rates -- runs gpz_poisson_nsf on its block of genes, and the gradients w.r.t. the moments return to the
 * latents' owners by gpz_reduce_scatter_sum_f32 (recv = this rank's n_per_rank block of the element-wise sum of every
 * rank's world * n_per_rank values; send and recv may not overlap); gpz_allreduce_sum_f32 sums replicated fp32
 * gradients (the size factors V) in place.  All asynchronous on `stream`. */
int gpz_allgather(void* comm, const void* send, void* recv, int64_t bytes_per_rank, void* stream);
int gpz_reduce_scatter_sum_f32(void* comm, const float* send, float* recv, int64_t n_per_rank, void* stream);
int gpz_allreduce_sum_f32(void* comm, float* buf, int64_t n, void* stream);
int gpz_comm_destroy(void* comm);

/* Timing hooks used by bench.py: HIP events recorded on `stream` around the
 * dominant kernels of the last gpz_svgp_forward call (roofline.achieved).  These events are the only HIP objects
 * the library ever creates (streams always come from the caller): gpz_profile_enable(1) starts recording,
 * gpz_profile_enable(0) stops and DESTROYS every event, so nothing of the library's outlives it at process exit. */
int gpz_profile_enable(int32_t on);
int gpz_profile_read(double* ms_out, int32_t* counts_out, int32_t n_slots); /* host arrays */

#ifdef __cplusplus
}
#endif
#endif /* GPZOO_HIP_H */
