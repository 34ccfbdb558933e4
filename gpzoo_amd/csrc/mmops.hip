// mmops.hip -- the (L,Mp,Mp) / (L,M,M) helpers declared in mmops.h: one kernel and one launcher each.
#include "mmops.h"
#include "gemm.h"
#include "kgrad.h"

#include <algorithm>

namespace gpz {

namespace {
// grids: 32 x 32 tiles of a padded matrix / one row of it per blockIdx.y
dim3 tiles32(int64_t Mp, int L) { return dim3((unsigned)(Mp / 32), (unsigned)(Mp / 32), (unsigned)L); }
dim3 rows256(int64_t cols, int64_t rows, int L) { return dim3((unsigned)((cols + 255) / 256), (unsigned)rows, (unsigned)L); }
}  // namespace

__global__ __launch_bounds__(256) void tril_transpose_kernel(const double* __restrict__ src, int64_t Mp,
                                                            double* __restrict__ dst) {
  __shared__ double tile[32][33];
  const int l = blockIdx.z;
  const int64_t i0 = (int64_t)blockIdx.y * 32, j0 = (int64_t)blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int rr = ty; rr < 32; rr += 8) {
    const int64_t i = i0 + rr, j = j0 + tx;
    tile[rr][tx] = (j <= i) ? src[(int64_t)l * Mp * Mp + i * Mp + j] : 0.0;
  }
  __syncthreads();
  for (int rr = ty; rr < 32; rr += 8) dst[(int64_t)l * Mp * Mp + (j0 + rr) * Mp + i0 + tx] = tile[tx][rr];
}

int tril_transpose(const double* src, int64_t Mp, int L, double* dst, hipStream_t s) {
  hipLaunchKernelGGL(tril_transpose_kernel, tiles32(Mp, L), dim3(256), 0, s, src, Mp, dst);
  GPZ_LAUNCH_OK();
  return 0;
}

__global__ void phi_kernel(double* __restrict__ A, int64_t Mp) {
  const int l = blockIdx.z;
  const int64_t i = blockIdx.y, j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= Mp) return;
  double& v = A[(int64_t)l * Mp * Mp + i * Mp + j];
  if (j > i) v = 0.0;
  else if (j == i) v *= 0.5;
}

int phi(double* A, int64_t Mp, int L, hipStream_t s) {
  hipLaunchKernelGGL(phi_kernel, rows256(Mp, Mp, L), dim3(256), 0, s, A, Mp);
  GPZ_LAUNCH_OK();
  return 0;
}

template <typename T>
__global__ __launch_bounds__(256) void sym_cast_kernel(const double* __restrict__ P, const double* __restrict__ Q,
                                                      int64_t Mp, T* __restrict__ dst) {
  __shared__ double tile[32][33];
  const int l = blockIdx.z;
  const int64_t i0 = (int64_t)blockIdx.y * 32, j0 = (int64_t)blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t base = (int64_t)l * Mp * Mp;
  for (int rr = ty; rr < 32; rr += 8) {
    const int64_t o = base + (j0 + rr) * Mp + i0 + tx;   // the transposed element
    tile[rr][tx] = Q ? P[o] + Q[o] : P[o];
  }
  __syncthreads();
  for (int rr = ty; rr < 32; rr += 8) {
    const int64_t o = base + (i0 + rr) * Mp + j0 + tx;
    dst[o] = (T)((Q ? P[o] + Q[o] : P[o]) + tile[tx][rr]);
  }
}

template <typename T>
int sym_cast(const double* P, const double* Q, int64_t Mp, int L, T* dst, hipStream_t s) {
  hipLaunchKernelGGL((sym_cast_kernel<T>), tiles32(Mp, L), dim3(256), 0, s, P, Q, Mp, dst);
  GPZ_LAUNCH_OK();
  return 0;
}

template <typename T>
__global__ __launch_bounds__(256) void lu_forward_kernel(const T* __restrict__ raw, int64_t M, int64_t Mp,
                                                        T* __restrict__ LuT, double* __restrict__ LuD,
                                                        T* __restrict__ LuOut, double* __restrict__ part,
                                                        T* __restrict__ LuN) {
  __shared__ double tile[32][33];
  __shared__ double sh[8];
  const int l = blockIdx.z;
  const int64_t i0 = (int64_t)blockIdx.y * 32, j0 = (int64_t)blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  double fro = 0.0, ld = 0.0;
  for (int rr = ty; rr < 32; rr += 8) {
    const int64_t i = i0 + rr, j = j0 + tx;
    double v = 0.0;
    if (i < M && j < M && j <= i) {
      const double x = (double)raw[(int64_t)l * M * M + i * M + j];
      if (i == j) { v = exp(x); ld += x; } else v = x;
      fro += v * v;
    }
    tile[rr][tx] = v;
    if (LuOut && i < M && j < M) LuOut[(int64_t)l * M * M + i * M + j] = (T)v;
    if (LuD && i < Mp && j < Mp) LuD[(int64_t)l * Mp * Mp + i * Mp + j] = v;
    if (LuN && i < Mp && j < Mp) LuN[(int64_t)l * Mp * Mp + i * Mp + j] = (T)v;   // padded, lower, not transposed
  }
  __syncthreads();
  if (LuT)
    for (int rr = ty; rr < 32; rr += 8) {
      const int64_t jt = j0 + rr, it = i0 + tx;  // LuT[j][i] = Lu[i][j]
      if (jt < Mp && it < Mp) LuT[(int64_t)l * Mp * Mp + jt * Mp + it] = (T)tile[tx][rr];
    }
  if (!part) return;
  const double f = block_sum(fro, sh);
  const double g = block_sum(ld, sh);
  if (threadIdx.x == 0) {
    const int64_t nb = (int64_t)gridDim.x * gridDim.y, b = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    part[((int64_t)l * 2 + 0) * nb + b] = f;
    part[((int64_t)l * 2 + 1) * nb + b] = g;
  }
}

template <typename T>
int lu_forward(const T* raw, int64_t M, int64_t Mp, int L, T* LuT, double* LuD, T* LuOut, double* part, T* LuN, hipStream_t s) {
  hipLaunchKernelGGL((lu_forward_kernel<T>), tiles32(Mp, L), dim3(256), 0, s, raw, M, Mp, LuT, LuD, LuOut, part, LuN);
  GPZ_LAUNCH_OK();
  return 0;
}

template <typename T, typename TG>
__global__ void lu_grad_kernel(const TG* __restrict__ G, int64_t Mp, int64_t M, const T* __restrict__ raw,
                               T* __restrict__ out, const double* __restrict__ g_kl, int whitened_kl) {
  const int l = blockIdx.z;
  const int64_t i = blockIdx.y, j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= M) return;
  double g = (double)G[(int64_t)l * Mp * Mp + i * Mp + j];
  const double gk = g_kl ? g_kl[l] : 0.0;
  const double x = (double)raw[(int64_t)l * M * M + i * M + j];
  T v = 0;
  if (j < i) {
    if (whitened_kl) g += gk * x;                 // whitened KL: d/dLu of |Lu|_F^2 / 2 (un-whitened: already in G)
    v = (T)g;
  } else if (j == i) {   // Lu_ii = exp(raw_ii); the KL's -log Lu_ii contributes -g_kl to the raw diagonal
    const double e = exp(x);
    if (whitened_kl) g += gk * e;
    v = (T)(g * e - gk);
  }
  out[(int64_t)l * M * M + i * M + j] = v;
}

template <typename T, typename TG>
int lu_grad(const TG* G, int64_t Mp, int64_t M, int L, const T* raw, T* out, const double* g_kl, int whitened_kl, hipStream_t s) {
  hipLaunchKernelGGL((lu_grad_kernel<T, TG>), rows256(M, M, L), dim3(256), 0, s, G, Mp, M, raw, out, g_kl, whitened_kl);
  GPZ_LAUNCH_OK();
  return 0;
}

// (one block per latent along x == 0 sums the log diagonal)
template <typename T>
__global__ __launch_bounds__(256) void chol_out_kernel(const double* __restrict__ Lc, int64_t Mp, int64_t M,
                                                      T* __restrict__ out, double* __restrict__ logdiag) {
  __shared__ double sh[8];
  const int l = blockIdx.y;
  const double* src = Lc + (int64_t)l * Mp * Mp;
  if (out) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < M * M; e += (int64_t)gridDim.x * 256) {
      const int64_t i = e / M, j = e - i * M;
      out[(int64_t)l * M * M + e] = (j <= i) ? (T)src[i * Mp + j] : (T)0;
    }
  }
  if (blockIdx.x == 0 && logdiag) {
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < M; i += 256) s += log(src[i * (Mp + 1)]);
    const double t = block_sum(s, sh);
    if (threadIdx.x == 0) logdiag[l] = t;
  }
}

template <typename T>
int chol_out(const double* Lc, int64_t Mp, int64_t M, int L, T* out, double* logdiag, hipStream_t s) {
  hipLaunchKernelGGL((chol_out_kernel<T>), dim3(out ? 64 : 1, (unsigned)L), dim3(256), 0, s, Lc, Mp, M, out, logdiag);
  GPZ_LAUNCH_OK();
  return 0;
}

template <typename T>
__global__ void tril_widen_kernel(const T* __restrict__ src, int64_t ld, int64_t Mp, double* __restrict__ dst) {
  const int l = blockIdx.z;
  const int64_t i = blockIdx.y, j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= Mp) return;
  dst[(int64_t)l * Mp * Mp + i * Mp + j] = (i < ld && j <= i) ? (double)src[(int64_t)l * ld * ld + i * ld + j] : 0.0;
}

template <typename T>
int tril_widen(const T* src, int64_t ld, int64_t Mp, int L, double* dst, hipStream_t s) {
  hipLaunchKernelGGL((tril_widen_kernel<T>), rows256(Mp, Mp, L), dim3(256), 0, s, src, ld, Mp, dst);
  GPZ_LAUNCH_OK();
  return 0;
}

// 32 columns x 8 row segments per block (a thread per column alone walks up to M rows serially: 0.73 ms at M = 3000,
// L = 20); outputs a < nout
template <typename TO>
__global__ __launch_bounds__(256) void linvT_vec_kernel(const double* __restrict__ v, const double* __restrict__ Linv,
                                                       int64_t Mp, int64_t M, TO* __restrict__ out, int64_t ldo,
                                                       int64_t nout, const double* __restrict__ g_kl) {
  __shared__ double sh[8][33];
  const int l = blockIdx.y, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t a = (int64_t)blockIdx.x * 32 + tx;
  const double* Lb = Linv + (int64_t)l * Mp * Mp;
  double t = 0.0;
  if (a < M)
    for (int64_t i = a + ty; i < M; i += 8) t = fma(Lb[i * Mp + a], v[(int64_t)l * Mp + i], t);
  sh[ty][tx] = t;
  __syncthreads();
  if (ty == 0 && a < nout) {
    double r = 0.0;
#pragma unroll
    for (int q = 0; q < 8; ++q) r += sh[q][tx];
    TO& o = out[(int64_t)l * ldo + a];
    if (g_kl) o += (TO)(g_kl[l] * r);
    else o = (TO)r;
  }
}

template <typename TO>
int linvT_vec(const double* v, const double* Linv, int64_t Mp, int64_t M, int L, TO* out, int64_t ldo, const double* g_kl,
              hipStream_t s) {
  GPZ_REQUIRE(!g_kl || (sizeof(TO) == 8 && ldo == Mp), "linvT_vec: the += g_kl r form is fp64 over (L, Mp)");
  const int64_t nout = g_kl ? M : ldo;
  hipLaunchKernelGGL((linvT_vec_kernel<TO>), dim3((unsigned)((nout + 31) / 32), (unsigned)L), dim3(256), 0, s, v, Linv, Mp,
                     M, out, ldo, nout, g_kl);
  GPZ_LAUNCH_OK();
  return 0;
}

__global__ __launch_bounds__(256) void kgrad_finish_kernel(const double* __restrict__ acc, int L, int64_t Mp, int64_t M,
                                                          int d, const double* __restrict__ sig_direct,
                                                          double* __restrict__ grad_Z, double* __restrict__ grad_theta) {
  __shared__ double sh[8];
  if (blockIdx.y == 0) {            // Z rows
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m < M && grad_Z)
      for (int k = 0; k < 4; ++k) {
        double t = 0.0;
        if (k < d)
          for (int l = 0; l < L; ++l) t += acc[((int64_t)l * Mp + m) * 8 + k];
        grad_Z[m * 4 + k] = t;
      }
  } else if ((int)blockIdx.x < L && grad_theta) {   // one block per latent
    const int l = blockIdx.x;
    for (int q = 0; q < 3; ++q) {
      double v = 0.0;
      for (int64_t m = threadIdx.x; m < M; m += 256) v += acc[((int64_t)l * Mp + m) * 8 + 4 + q];
      const double t = block_sum(v, sh);
      if (threadIdx.x == 0) grad_theta[l * 4 + q] = t + (q == 0 && sig_direct ? sig_direct[l] : 0.0);
    }
    if (threadIdx.x == 0) grad_theta[l * 4 + 3] = 0.0;
  }
}

int kgrad_finish(const double* acc, int L, int64_t Mp, int64_t M, int d, const double* sig_direct, double* grad_Z,
                 double* grad_theta, hipStream_t s) {
  const unsigned fx = (unsigned)std::max<int64_t>((M + 255) / 256, L);
  hipLaunchKernelGGL(kgrad_finish_kernel, dim3(fx, 2), dim3(256), 0, s, acc, L, Mp, M, d, sig_direct, grad_Z, grad_theta);
  GPZ_LAUNCH_OK();
  return 0;
}

int dgemm_mm(const double* A, const double* B, double* C, int64_t Mp, int L, int flags, double alpha, hipStream_t s) {
  const int64_t mm = Mp * Mp;
  GemmParams<double> d;
  d.A = A; d.lda = Mp; d.sA0 = mm; d.B = B; d.ldb = Mp; d.sB0 = mm; d.C = C; d.ldc = Mp; d.sC0 = mm;
  d.nb0 = L; d.mt = d.nt = (int)(Mp / 128); d.K = (int)Mp; d.flags = flags; d.alpha = alpha;
  return gemm_launch(d, EPI_STORE, s);
}

int chol_backward(const double* Lfac, const double* Linv, double* Lbar, int64_t Mp, int L, double* tmp, double* P,
                  hipStream_t s) {
  if (int rc = tril_transpose(Lfac, Mp, L, tmp, s)) return rc;                                          // tmp  = L^T
  if (int rc = dgemm_mm(tmp, Lbar, P, Mp, L, GF_A_UPPER | GF_B_LOWER, 1.0, s)) return rc;               // P    = L^T Lbar
  if (int rc = phi(P, Mp, L, s)) return rc;
  GPZ_HIP_OK(hipMemsetAsync(Lbar, 0, sizeof(double) * L * Mp * Mp, s));
  if (int rc = dgemm_mm(P, Linv, Lbar, Mp, L, GF_A_LOWER | GF_B_LOWER | GF_TILES_LOWER, 1.0, s)) return rc;   // Lbar = Phi Linv
  if (int rc = tril_transpose(Linv, Mp, L, tmp, s)) return rc;                                          // tmp  = Linv^T
  return dgemm_mm(tmp, Lbar, P, Mp, L, GF_A_UPPER | GF_B_LOWER, 1.0, s);                                // P    = Linv^T Phi Linv
}

int kzz_grad(const gpz_svgp_problem* p, const double* P, const double* Q, int64_t Mp, void* PS, double* kacc,
             const double* sig_direct, const gpz_svgp_grads* g, hipStream_t s) {
  const int L = p->k.n_latent;
  const int64_t M = p->M;
  if (int rc = p->dtype == GPZ_F32 ? sym_cast(P, Q, Mp, L, static_cast<float*>(PS), s)
                                   : sym_cast(P, Q, Mp, L, static_cast<double*>(PS), s))
    return rc;
  KgradArgs ka;
  ka.Kbar = PS; ka.ld = Mp; ka.stride = Mp * Mp; ka.Z = p->Z; ka.X = p->Z; ka.gZ = p->gZ; ka.gX = p->gZ;
  ka.sigma = p->k.sigma; ka.ell = p->k.lengthscale; ka.ga = p->k.group_a; ka.gr2 = p->k.group_r2;
  ka.gpow = p->k.group_pow; ka.scalar_scale = 0.5; ka.M = M; ka.ncols = M; ka.Mp = Mp; ka.d = p->d;
  ka.G = p->k.n_groups; ka.acc = kacc;
  if (int rc = kgrad_launch(p->dtype, p->k.kind, ka, L, s)) return rc;
  return kgrad_finish(kacc, L, Mp, M, p->d, sig_direct, g->grad_Z, g->grad_theta, s);
}

#define GPZ_MMOPS_INSTANCES(T)                                                                                          \
  template int sym_cast<T>(const double*, const double*, int64_t, int, T*, hipStream_t);                                \
  template int lu_forward<T>(const T*, int64_t, int64_t, int, T*, double*, T*, double*, T*, hipStream_t);               \
  template int lu_grad<T, T>(const T*, int64_t, int64_t, int, const T*, T*, const double*, int, hipStream_t);           \
  template int chol_out<T>(const double*, int64_t, int64_t, int, T*, double*, hipStream_t);                             \
  template int tril_widen<T>(const T*, int64_t, int64_t, int, double*, hipStream_t);                                    \
  template int linvT_vec<T>(const double*, const double*, int64_t, int64_t, int, T*, int64_t, const double*, hipStream_t);
GPZ_MMOPS_INSTANCES(float)
GPZ_MMOPS_INSTANCES(double)
#undef GPZ_MMOPS_INSTANCES
template int lu_grad<float, double>(const double*, int64_t, int64_t, int, const float*, float*, const double*, int, hipStream_t);

}  // namespace gpz
