// mmops.h -- the small fp64 "M x M plumbing" around the inducing-point factor that the SVGP backward (svgp.hip), the
// VNNGP forward / backward (vnngp.hip) and gpz_kgrad (kgrad.hip) share: transposes, casts, the Lu constraint and its
// chain rule, Linv^T v, the batched square fp64 product, the Cholesky backward and the contraction of its result with
// the kernel derivatives.  Matrices are (L, Mp, Mp) row-major, Mp = pad_up(M), unless a comment says (L, M, M); the
// launchers pick the grids.  T is float or double (instantiated in mmops.hip).
#pragma once
#include "common.h"

namespace gpz {

// Sum of v over the block on thread 0 (fixed-shape tree: lanes -> waves in order; deterministic).  sh: one double per wave.
__device__ __forceinline__ double block_sum(double v, double* sh) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[w] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += sh[i];
  return t;  // valid on thread 0
}

// dst = transpose(tril(src)), fp64 (src may hold garbage above the diagonal)
int tril_transpose(const double* src, int64_t Mp, int L, double* dst, hipStream_t s);
// Phi of the Cholesky backward (Murray 2016), in place: keep the lower triangle, halve the diagonal
int phi(double* A, int64_t Mp, int L, hipStream_t s);
// dst = (T)(P + P^T) or, with Q, (T)((P + Q) + (P + Q)^T).  Without Q nothing is added to P (a pair of -0.0 stays -0.0).
template <typename T>
int sym_cast(const double* P, const double* Q, int64_t Mp, int L, T* dst, hipStream_t s);

// Constrained scale_tril of q(U) from the raw parameter (L,M,M) (gp.py:220/278: strict lower triangle kept, diagonal
// exponentiated), emitted in up to four forms, each nullable:
//   LuT   (L,Mp,Mp) T   transposed (upper triangular), zero padded      [whitened: the stage-2 operand]
//   LuD   (L,Mp,Mp) f64 as is (lower triangular), zero padded           [un-whitened: input to Linv * Lu; VNNGP: S = Lu Lu^T]
//   LuOut (L,M,M)   T   for MultivariateNormal(scale_tril=...)
//   LuN   (L,Mp,Mp) T   as is, zero padded
// and, with `part` [L][2][(Mp/32)^2], per-block partial sums of ||Lu||_F^2 and of the raw diagonal (= log diag Lu).
template <typename T>
int lu_forward(const T* raw, int64_t M, int64_t Mp, int L, T* LuT, double* LuD, T* LuOut, double* part, T* LuN, hipStream_t s);
// chain rule of that constraint: out (L,M,M) from G = dLoss/dLu (TG: T or double).  g_kl (nullable, per latent) adds the
// KL's -log Lu_ii share of the raw diagonal and, with whitened_kl, its |Lu|_F^2 / 2 share (un-whitened: already in G)
template <typename T, typename TG>
int lu_grad(const TG* G, int64_t Mp, int64_t M, int L, const T* raw, T* out, const double* g_kl, int whitened_kl, hipStream_t s);

// Cholesky factor out: out (L,M,M) T with zeros above the diagonal, and sum(log diag) per latent; each nullable
template <typename T>
int chol_out(const double* Lc, int64_t Mp, int64_t M, int L, T* out, double* logdiag, hipStream_t s);
// dst (L,Mp,Mp) f64 = tril(src), src (L,ld,ld) with ld = Mp or M (then zero padded)
template <typename T>
int tril_widen(const T* src, int64_t ld, int64_t Mp, int L, double* dst, hipStream_t s);

// r[l][a] = sum_{i >= a} Linv[l][i][a] v[l][i]  (Linv^T v; v (L,Mp) f64), a < M.  Without g_kl: out[l][a] = (TO)r over
// (L,ldo), ldo = M, or ldo = Mp with zeros in the padding.  With g_kl (TO = double, ldo = Mp): out[l][a] += g_kl[l] r.
template <typename TO>
int linvT_vec(const double* v, const double* Linv, int64_t Mp, int64_t M, int L, TO* out, int64_t ldo, const double* g_kl,
              hipStream_t s);

// grad_Z[m][k] = sum_l acc[l][m][k];  grad_theta[l][0..2] = sum_m acc[l][m][4..6] (+ sig_direct[l] on [0], nullable),
// grad_theta[l][3] = 0; acc (L,Mp,8) as kgrad.hip leaves it
int kgrad_finish(const double* acc, int L, int64_t Mp, int64_t M, int d, const double* sig_direct, double* grad_Z,
                 double* grad_theta, hipStream_t s);

// C = alpha * A op(B): the batched square fp64 product over (L,Mp,Mp) (flags: GemmFlags of gemm.h)
int dgemm_mm(const double* A, const double* B, double* C, int64_t Mp, int L, int flags, double alpha, hipStream_t s);

// Cholesky backward (Murray 2016): P = Linv^T Phi(Lfac^T Lbar) Linv.  Lbar is overwritten, tmp is one more matrix.
int chol_backward(const double* Lfac, const double* Linv, double* Lbar, int64_t Mp, int L, double* tmp, double* P,
                  hipStream_t s);

// The Kzz tail of a backward pass: PS = P + P^T (+ Q + Q^T, Q nullable) in the problem's dtype, contracted with
// dKzz/d(sigma, lengthscale, a, Z) into kacc (scalars halved: PS counts every pair twice), then kgrad_finish into g.
// The group fields of the problem (gZ, group_a, group_r2, group_pow, n_groups) go into KgradArgs as they are: only the
// multi-group kind reads them, and VNNGP, which admits no such kind, may leave them unset.
int kzz_grad(const gpz_svgp_problem* p, const double* P, const double* Q, int64_t Mp, void* PS, double* kacc,
             const double* sig_direct, const gpz_svgp_grads* g, hipStream_t s);

}  // namespace gpz
