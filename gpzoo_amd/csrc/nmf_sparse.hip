// nmf_sparse.hip -- the KL multiplicative-update NMF of nmf.hip for counts stored as their non-zeros, and the two
// products of the counts with a thin dense matrix that its NNDSVD start needs.
//
//   X (N spots, D genes) >= 0, X[n,d] = counts[d,n]  ~  W (N,L) . H (L,D).  Q = X / max(W H, EPS) is zero wherever X is, so
//   both numerators of an iteration are sums over the non-zeros and the denominators are sums of the factors:
//     W pass, spot n, over its non-zeros k = (d_k, x_k):   p = sum_l W[n,l] H[l,d_k], q = x_k / max(p, EPS),
//             W[n,l] *= (sum_k q H[l,d_k]) / rowsum(H)[l]                         (a zero rowsum reads as EPS)
//     H pass, gene d, over its non-zeros k = (n_k, x_k), with the NEW W:
//             H[l,d] *= (sum_k q W[n_k,l]) / colsum(W)[l]                         (a zero colsum reads as 1);  H < eps64 -> 0
//   and the divergence is sum_{x > EPS} x log(x / max(p, EPS)) + colsum(W) . rowsum(H) - sum_{x > EPS} x.
// That is O(nnz L) per iteration; nothing of N x D elements and nothing of nnz elements exists, workspace included.
//
// The counts arrive in the two orders of gpzoo_amd.likelihoods.SparseCounts (poisson_sparse.hip): by spot (col_ptr,
// col_gene, col_val) = the non-zeros of a row of X, which the W pass reads, and by gene (row_ptr, row_spot, row_perm) = the
// non-zeros of a column of X, which the H pass reads.
//
// The hot loop gathers one factor row of L values per non-zero.  Both gathered tables are kept as padded row-major copies
// in the workspace, HT (D, LT) = H transposed and WP (N, LT) = W, LT = L padded to the kernel instance with zeros: a
// gathered row is one contiguous 16-byte aligned run.  HT is built once per call and refreshed by the H update, WP is
// written by the W update; they are L2-sized at Slide-seq size (1.7 MB and 3.8 MB in fp32 at L = 20).
//
// Launches of one iteration (fp32 or fp64, fp64 for the factor sums; no atomics, no workgroup waits on another, every sum
// in a fixed order -> two calls agree bit for bit, 2 k iterations equal k + k):
//   ns_colsum_kernel + ns_colsum_final_kernel   rowsum(H) = column sums of HT: partials per 256 rows, added in ascending order
//   ns_spot_kernel<UPDATE>   one wave per spot; W[n,:] is wave-uniform, lanes stride over the spot's non-zeros with per-lane
//                            accumulators, one fixed cross-lane tree per factor finishes the row; writes W and WP
//   ns_colsum_kernel + ns_colsum_final_kernel   colsum(W) from WP
//   ns_gene_kernel           one wave per (gene, chunk of 512 consecutive non-zeros): the chunk's partial numerator
//   ns_h_finish_kernel       adds a gene's chunk partials in chunk order, applies the update to H and HT
// Once per call: ns_transpose_kernel (H -> HT) and chunks_kernel (the gene pass's work list).  A spot's row has at most
// D entries and spots are of similar depth, so spot rows are not cut (as in poisson_sparse.hip).
//
// gpz_counts_matmul (fp64) is the same wave per spot / per (gene, chunk) with the lanes across the k <= 128 columns of Q:
// every stored value is broadcast in its stored order and each lane adds x Q[row, j] to its own columns -- a coalesced row
// read per non-zero, no cross-lane sum at all; chunk partials are added in chunk order.
#include <math.h>

#include "common.h"
#include "sparse_rows.h"

namespace gpz {
namespace {

constexpr int NS_LMAX = 64;       // factors
constexpr int NS_KMAX = 128;      // columns of Q in gpz_counts_matmul
constexpr int NS_CHUNK = 512;     // non-zeros of one gene row per wave of the gene pass
constexpr int NS_ROWS = 256;      // rows per workgroup of ns_colsum_kernel
#define NS_EPS 1.1920928955078125e-07     // np.finfo(np.float32).eps, in both precisions
#define NS_EPS64 2.220446049250313e-16    // np.finfo(np.float64).eps

typedef float nf32x4 __attribute__((ext_vector_type(4)));
typedef double nf64x2 __attribute__((ext_vector_type(2)));

struct NsCounts {
  const int64_t* col_ptr; const int32_t* col_gene; const float* col_val;
  const int64_t* row_ptr; const int32_t* row_spot; const int32_t* row_perm;
};

template <typename T>
struct NsArgs {
  NsCounts c;
  T *W, *H;                       // (N, L), (L, D): the caller's
  T *HT, *WP;                     // (D, LT), (N, LT)
  double *hpart, *wpart;          // [nbD][LT], [nbN][LT]
  double *hsum, *wsum;            // [64]
  double *dspot, *dpart, *dtot;   // [N][2], [nbN][2], [2]: the divergence's two sums
  int32_t *cstart, *chunk_gene;   // [D + 1], [nchunks]
  T* part;                        // [nchunks][LT]
  int64_t N, D, nnz, nchunks;
  int L, LT, nbN, nbD;
};

int ns_instance(int L) {
  const int sizes[] = {4, 8, 12, 16, 20, 24, 32, 40, 48, 64};
  for (int s : sizes) if (L <= s) return s;
  return 0;
}

// a padded factor row (LT a multiple of 4, the row 16-byte aligned)
template <int LT>
__device__ __forceinline__ void ns_load_row(const float* p, float (&v)[LT]) {
#pragma unroll
  for (int l = 0; l < LT; l += 4) {
    const nf32x4 t = *reinterpret_cast<const nf32x4*>(p + l);
    v[l] = t[0]; v[l + 1] = t[1]; v[l + 2] = t[2]; v[l + 3] = t[3];
  }
}
template <int LT>
__device__ __forceinline__ void ns_load_row(const double* p, double (&v)[LT]) {
#pragma unroll
  for (int l = 0; l < LT; l += 2) {
    const nf64x2 t = *reinterpret_cast<const nf64x2*>(p + l);
    v[l] = t[0]; v[l + 1] = t[1];
  }
}

template <typename T, int LT>
__device__ __forceinline__ T ns_dot_clamped(const T (&a)[LT], const T (&b)[LT]) {
  T z = T(0);
#pragma unroll
  for (int l = 0; l < LT; ++l) z = a[l] * b[l] + z;
  return z < T(NS_EPS) ? T(NS_EPS) : z;
}

// HT[d][l] = H[l][d] for l < L, zero for L <= l < LT.  Workgroup = 64 genes.
template <typename T>
__global__ __launch_bounds__(256) void ns_transpose_kernel(const T* __restrict__ H, int64_t D, int L, int LT, T* __restrict__ HT) {
  __shared__ T xt[NS_LMAX][65];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t d0 = (int64_t)blockIdx.x * 64, d = d0 + lane;
  for (int l = wave; l < LT; l += 4) xt[l][lane] = (l < L && d < D) ? H[(int64_t)l * D + d] : T(0);
  __syncthreads();
  for (int i = threadIdx.x; i < 64 * LT; i += 256) {
    const int jj = i / LT, l = i - jj * LT;
    if (d0 + jj < D) HT[(d0 + jj) * LT + l] = xt[l][jj];
  }
}

// part[b][l] = sum over rows b * 256 ... of src[row * stride + l] (l < ncols; zero beyond, l < LT), in fp64 and a fixed order
template <typename T>
__global__ __launch_bounds__(256) void ns_colsum_kernel(const T* __restrict__ src, int64_t R, int stride, int ncols, int LT,
                                                        double* __restrict__ part) {
  __shared__ double sh[4][64];
  const int l = threadIdx.x & 63, r = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * NS_ROWS, r1 = r0 + NS_ROWS < R ? r0 + NS_ROWS : R;
  double v = 0.0;
  if (l < ncols) {
#pragma unroll 8
    for (int64_t row = r0 + r; row < r1; row += 4) v += (double)src[row * stride + l];
  }
  sh[r][l] = v;
  __syncthreads();
  if (r == 0 && l < LT) part[(int64_t)blockIdx.x * LT + l] = (sh[0][l] + sh[1][l]) + (sh[2][l] + sh[3][l]);
}

// out[l] = sum_b part[b][l] in ascending b (one workgroup of 64 threads)
__global__ __launch_bounds__(64) void ns_colsum_final_kernel(const double* __restrict__ part, int nb, int LT, double* __restrict__ out) {
  const int l = threadIdx.x;
  if (l >= LT) return;
  double v = 0.0;
#pragma unroll 8
  for (int b = 0; b < nb; ++b) v += part[(int64_t)b * LT + l];
  out[l] = v;
}

// Spot pass.  4 waves per workgroup, wave = spot n; no barrier, so a wave without a spot leaves at once.
// UPDATE: the W update of spot n, written to W and to WP (zeros beyond L).  Otherwise the spot's two sums of the divergence.
template <typename T, int LT, bool UPDATE>
__global__ __launch_bounds__(256) void ns_spot_kernel(NsArgs<T> a) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t n = (int64_t)blockIdx.x * 4 + wave;
  if (n >= a.N) return;
  const int64_t k0 = a.c.col_ptr[n], k1 = a.c.col_ptr[n + 1];
  T w[LT];
#pragma unroll
  for (int l = 0; l < LT; ++l) w[l] = l < a.L ? a.W[n * a.L + l] : T(0);
  T acc[LT];
#pragma unroll
  for (int l = 0; l < LT; ++l) acc[l] = T(0);
  double dv = 0.0, dx = 0.0;
  for (int64_t k = k0 + lane; k < k1; k += 64) {
    const T x = T(a.c.col_val[k]);
    T h[LT];
    ns_load_row<LT>(a.HT + (int64_t)a.c.col_gene[k] * LT, h);
    const T p = ns_dot_clamped<T, LT>(w, h);
    if (UPDATE) {
      const T q = x / p;
#pragma unroll
      for (int l = 0; l < LT; ++l) acc[l] = q * h[l] + acc[l];
    } else if (x > T(NS_EPS)) {
      dv += double(x) * log(double(x) / double(p));
      dx += double(x);
    }
  }
  if (UPDATE) {
    T mine = T(0);
#pragma unroll
    for (int l = 0; l < LT; ++l) {
      const T t = wave_sum(acc[l]);
      if (lane == l) mine = t;
    }
    if (lane < LT) {
      T out = T(0);
      if (lane < a.L) {
        T den = T(a.hsum[lane]);
        if (den == T(0)) den = T(NS_EPS);
        out = a.W[n * a.L + lane] * (mine / den);
        a.W[n * a.L + lane] = out;
      }
      a.WP[n * LT + lane] = out;
    }
  } else {
    dv = wave_sum(dv);
    dx = wave_sum(dx);
    if (lane == 0) {
      a.dspot[2 * n] = dv;
      a.dspot[2 * n + 1] = dx;
    }
  }
}

// Gene pass.  4 waves per workgroup, wave = chunk w of the work list: at most 512 consecutive non-zeros of one gene row.
template <typename T, int LT>
__global__ __launch_bounds__(256) void ns_gene_kernel(NsArgs<T> a) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t wi = (int64_t)blockIdx.x * 4 + wave;
  if (wi >= a.nchunks) return;
  const int g = a.chunk_gene[wi];
  if (g < 0) return;
  const int64_t p0 = a.c.row_ptr[g] + (wi - a.cstart[g]) * NS_CHUNK;
  const int64_t pe = a.c.row_ptr[g + 1], p1 = p0 + NS_CHUNK < pe ? p0 + NS_CHUNK : pe;
  T h[LT], acc[LT];
  ns_load_row<LT>(a.HT + (int64_t)g * LT, h);
#pragma unroll
  for (int l = 0; l < LT; ++l) acc[l] = T(0);
  for (int64_t p = p0 + lane; p < p1; p += 64) {
    const T x = T(a.c.col_val[a.c.row_perm[p]]);
    T wv[LT];
    ns_load_row<LT>(a.WP + (int64_t)a.c.row_spot[p] * LT, wv);
    const T q = x / ns_dot_clamped<T, LT>(wv, h);
#pragma unroll
    for (int l = 0; l < LT; ++l) acc[l] = q * wv[l] + acc[l];
  }
  T mine = T(0);
#pragma unroll
  for (int l = 0; l < LT; ++l) {
    const T t = wave_sum(acc[l]);
    if (lane == l) mine = t;
  }
  if (lane < LT) a.part[wi * LT + lane] = mine;
}

// H[l][d] *= (sum of the gene's chunk partials in chunk order) / colsum(W)[l];  H < eps64 -> 0; H and HT both written.
template <typename T>
__global__ __launch_bounds__(256) void ns_h_finish_kernel(NsArgs<T> a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.D * a.LT) return;
  const int64_t d = i / a.LT;
  const int l = (int)(i - d * a.LT);
  if (l >= a.L) return;                    // the padding of HT holds zeros since ns_transpose_kernel
  double s = 0.0;
  for (int64_t c = a.cstart[d]; c < a.cstart[d + 1]; ++c) s += double(a.part[c * a.LT + l]);
  T den = T(a.wsum[l]);
  if (den == T(0)) den = T(1);
  T h = a.HT[i] * (T(s) / den);
  if (h < T(NS_EPS64)) h = T(0);
  a.HT[i] = h;
  a.H[(int64_t)l * a.D + d] = h;
}

// sqrt(2 max(res, 0)), res = sum x log(x / p) + colsum(W) . rowsum(H) - sum x
__global__ __launch_bounds__(64) void ns_div_final_kernel(const double* __restrict__ dtot, const double* __restrict__ wsum,
                                                          const double* __restrict__ hsum, int L, double* __restrict__ out) {
  if (threadIdx.x != 0) return;
  double swh = 0.0;
  for (int l = 0; l < L; ++l) swh += wsum[l] * hsum[l];
  double res = dtot[0] + (swh - dtot[1]);
  if (!(res > 0.0)) res = res != res ? res : 0.0;
  *out = sqrt(2.0 * res);
}

// ---- counts x Q -------------------------------------------------------------------------------------------------------

struct NsMatArgs {
  NsCounts c;
  const double* Q;
  double *out, *part;             // (rows, k); [nchunks][k]
  int32_t *cstart, *chunk_gene;
  int64_t N, D, nnz, nchunks;
  int k;
};

// BY_GENE = false: wave = spot n, out[n][:] = sum over the spot's non-zeros of x Q[d][:]                 (X Q)
// BY_GENE = true:  wave = chunk w of gene g, part[w][:] = sum over the chunk's non-zeros of x Q[n][:]    (X^T Q)
// Lane j owns columns j and j + 64; the non-zeros are taken 64 at a time and broadcast in their stored order.
template <bool BY_GENE>
__global__ __launch_bounds__(256) void ns_matmul_kernel(NsMatArgs a) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t wi = (int64_t)blockIdx.x * 4 + wave;
  int64_t p0, p1;
  if (BY_GENE) {
    if (wi >= a.nchunks) return;
    const int g = a.chunk_gene[wi];
    if (g < 0) return;
    p0 = a.c.row_ptr[g] + (wi - a.cstart[g]) * NS_CHUNK;
    const int64_t pe = a.c.row_ptr[g + 1];
    p1 = p0 + NS_CHUNK < pe ? p0 + NS_CHUNK : pe;
  } else {
    if (wi >= a.N) return;
    p0 = a.c.col_ptr[wi];
    p1 = a.c.col_ptr[wi + 1];
  }
  const bool has0 = lane < a.k, has1 = lane + 64 < a.k;
  double acc0 = 0.0, acc1 = 0.0;
  for (int64_t pb = p0; pb < p1; pb += 64) {
    const int64_t p = pb + lane;
    int row = 0;
    double x = 0.0;
    if (p < p1) {
      row = BY_GENE ? a.c.row_spot[p] : a.c.col_gene[p];
      x = double(a.c.col_val[BY_GENE ? (int64_t)a.c.row_perm[p] : p]);
    }
    const int cnt = p1 - pb < 64 ? (int)(p1 - pb) : 64;
    for (int i = 0; i < cnt; ++i) {
      const double* q = a.Q + (int64_t)__shfl(row, i) * a.k;
      const double xv = __shfl(x, i);
      if (has0) acc0 += xv * q[lane];
      if (has1) acc1 += xv * q[lane + 64];
    }
  }
  double* o = (BY_GENE ? a.part : a.out) + wi * a.k;
  if (has0) o[lane] = acc0;
  if (has1) o[lane + 64] = acc1;
}

// out[d][j] = sum of gene d's chunk partials in chunk order
__global__ __launch_bounds__(256) void ns_matmul_finish_kernel(NsMatArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.D * a.k) return;
  const int64_t d = i / a.k;
  const int j = (int)(i - d * a.k);
  double s = 0.0;
  for (int64_t c = a.cstart[d]; c < a.cstart[d + 1]; ++c) s += a.part[c * a.k + j];
  a.out[i] = s;
}

// ---- host -------------------------------------------------------------------------------------------------------------

int ns_check_counts(const char* who, int64_t N, int64_t D, int64_t nnz) {
  GPZ_REQUIRE(N >= 1 && D >= 1 && nnz >= 0, "%s: bad extents (N = %lld, D = %lld, nnz = %lld)", who, (long long)N, (long long)D,
              (long long)nnz);
  GPZ_REQUIRE(N < (1ll << 31) && D < (1ll << 31) && nnz < (1ll << 31) && D + nnz / NS_CHUNK < (1ll << 31),
              "%s: spots, genes and non-zeros are indexed with 32 bits (N = %lld, D = %lld, nnz = %lld)", who, (long long)N,
              (long long)D, (long long)nnz);
  return 0;
}

int ns_check_shape(const char* who, int64_t N, int64_t D, int64_t nnz, int L, int32_t dtype) {
  GPZ_REQUIRE(dtype == GPZ_F32 || dtype == GPZ_F64, "%s: unknown dtype %d", who, dtype);
  GPZ_REQUIRE(L >= 1 && L <= NS_LMAX, "%s: L=%d unsupported (1..%d)", who, L, NS_LMAX);
  return ns_check_counts(who, N, D, nnz);
}

int ns_check_pointers(const char* who, const NsCounts& c, int64_t nnz, const void* ws) {
  GPZ_REQUIRE(c.col_ptr && c.row_ptr && ws, "%s: null pointer", who);
  GPZ_REQUIRE(nnz == 0 || (c.col_gene && c.col_val && c.row_spot && c.row_perm), "%s: null pointer (non-zeros)", who);
  GPZ_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "%s: the workspace must be 16-byte aligned", who);
  return 0;
}

struct NsPlan { int LT, nbN, nbD; int64_t nchunks; size_t bytes; };

template <typename T>
NsPlan ns_plan(int64_t N, int64_t D, int64_t nnz, int L, NsArgs<T>* a, void* ws) {
  NsPlan p;
  p.LT = ns_instance(L);
  p.nbN = (int)((N + NS_ROWS - 1) / NS_ROWS);
  p.nbD = (int)((D + NS_ROWS - 1) / NS_ROWS);
  p.nchunks = D + nnz / NS_CHUNK;            // sum_d ceil(len_d / C) <= D + floor(nnz / C)
  Carver c(ws);
  T* HT = c.take<T>((size_t)D * p.LT);
  T* WP = c.take<T>((size_t)N * p.LT);
  double* hpart = c.take<double>((size_t)p.nbD * p.LT);
  double* wpart = c.take<double>((size_t)p.nbN * p.LT);
  double* hsum = c.take<double>(NS_LMAX);
  double* wsum = c.take<double>(NS_LMAX);
  double* dspot = c.take<double>((size_t)N * 2);
  double* dpart = c.take<double>((size_t)p.nbN * 2);
  double* dtot = c.take<double>(2);
  int32_t* cstart = c.take<int32_t>((size_t)D + 1);
  int32_t* chunk_gene = c.take<int32_t>((size_t)p.nchunks);
  T* part = c.take<T>((size_t)p.nchunks * p.LT);
  p.bytes = c.used();
  if (a) {
    a->HT = HT; a->WP = WP; a->hpart = hpart; a->wpart = wpart; a->hsum = hsum; a->wsum = wsum; a->dspot = dspot; a->dpart = dpart;
    a->dtot = dtot; a->cstart = cstart; a->chunk_gene = chunk_gene; a->part = part;
    a->N = N; a->D = D; a->nnz = nnz; a->nchunks = p.nchunks; a->L = L; a->LT = p.LT; a->nbN = p.nbN; a->nbD = p.nbD;
  }
  return p;
}

size_t ns_plan_bytes(int64_t N, int64_t D, int64_t nnz, int L, int32_t dtype) {
  return dtype == GPZ_F32 ? ns_plan<float>(N, D, nnz, L, nullptr, nullptr).bytes : ns_plan<double>(N, D, nnz, L, nullptr, nullptr).bytes;
}

template <typename T>
int ns_colsum(const T* src, int64_t R, int stride, int ncols, int LT, int nb, double* part, double* out, hipStream_t s) {
  hipLaunchKernelGGL((ns_colsum_kernel<T>), dim3((unsigned)nb), dim3(256), 0, s, src, R, stride, ncols, LT, part);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(ns_colsum_final_kernel, dim3(1), dim3(64), 0, s, part, nb, LT, out);
  GPZ_LAUNCH_OK();
  return 0;
}

template <typename T>
int ns_prologue(const NsArgs<T>& a, bool chunks, hipStream_t s) {
  hipLaunchKernelGGL((ns_transpose_kernel<T>), dim3((unsigned)((a.D + 63) / 64)), dim3(256), 0, s, a.H, a.D, a.L, a.LT, a.HT);
  GPZ_LAUNCH_OK();
  if (chunks) {
    hipLaunchKernelGGL(chunks_kernel, dim3(1), dim3(1024), 0, s, a.c.row_ptr, a.D, a.nchunks, NS_CHUNK, false, a.cstart, a.chunk_gene);
    GPZ_LAUNCH_OK();
  }
  return 0;
}

template <typename T, int LT>
int ns_iterate(const NsArgs<T>& a, int64_t iters, hipStream_t s) {
  if (int rc = ns_prologue<T>(a, true, s)) return rc;
  const dim3 spots((unsigned)((a.N + 3) / 4)), chunks((unsigned)((a.nchunks + 3) / 4));
  for (int64_t it = 0; it < iters; ++it) {
    if (int rc = ns_colsum<T>(a.HT, a.D, LT, LT, LT, a.nbD, a.hpart, a.hsum, s)) return rc;
    hipLaunchKernelGGL((ns_spot_kernel<T, LT, true>), spots, dim3(256), 0, s, a);
    GPZ_LAUNCH_OK();
    if (int rc = ns_colsum<T>(a.WP, a.N, LT, LT, LT, a.nbN, a.wpart, a.wsum, s)) return rc;
    hipLaunchKernelGGL((ns_gene_kernel<T, LT>), chunks, dim3(256), 0, s, a);
    GPZ_LAUNCH_OK();
    hipLaunchKernelGGL((ns_h_finish_kernel<T>), dim3((unsigned)((a.D * LT + 255) / 256)), dim3(256), 0, s, a);
    GPZ_LAUNCH_OK();
  }
  return 0;
}

template <typename T, int LT>
int ns_divergence(const NsArgs<T>& a, double* out, hipStream_t s) {
  if (int rc = ns_prologue<T>(a, false, s)) return rc;
  if (int rc = ns_colsum<T>(a.HT, a.D, LT, LT, LT, a.nbD, a.hpart, a.hsum, s)) return rc;
  if (int rc = ns_colsum<T>(a.W, a.N, a.L, a.L, LT, a.nbN, a.wpart, a.wsum, s)) return rc;
  hipLaunchKernelGGL((ns_spot_kernel<T, LT, false>), dim3((unsigned)((a.N + 3) / 4)), dim3(256), 0, s, a);
  GPZ_LAUNCH_OK();
  if (int rc = ns_colsum<double>(a.dspot, a.N, 2, 2, 2, a.nbN, a.dpart, a.dtot, s)) return rc;
  hipLaunchKernelGGL(ns_div_final_kernel, dim3(1), dim3(64), 0, s, a.dtot, a.wsum, a.hsum, a.L, out);
  GPZ_LAUNCH_OK();
  return 0;
}

#define NS_DISPATCH(T, LT_, CALL)          \
  switch (LT_) {                           \
    case 4: return CALL(T, 4);             \
    case 8: return CALL(T, 8);             \
    case 12: return CALL(T, 12);           \
    case 16: return CALL(T, 16);           \
    case 20: return CALL(T, 20);           \
    case 24: return CALL(T, 24);           \
    case 32: return CALL(T, 32);           \
    case 40: return CALL(T, 40);           \
    case 48: return CALL(T, 48);           \
    default: return CALL(T, 64);           \
  }

template <typename T>
int ns_iterate_any(const NsArgs<T>& a, int64_t iters, hipStream_t s) {
#define NS_CALL_IT(T_, LT_) ns_iterate<T_, LT_>(a, iters, s)
  NS_DISPATCH(T, a.LT, NS_CALL_IT);
#undef NS_CALL_IT
}

template <typename T>
int ns_divergence_any(const NsArgs<T>& a, double* out, hipStream_t s) {
#define NS_CALL_DIV(T_, LT_) ns_divergence<T_, LT_>(a, out, s)
  NS_DISPATCH(T, a.LT, NS_CALL_DIV);
#undef NS_CALL_DIV
}

template <typename T>
int ns_run(const char* who, const NsCounts& c, void* W, void* H, int64_t N, int64_t D, int64_t nnz, int L, int64_t iters,
           double* out, void* ws, size_t ws_bytes, hipStream_t s) {
  NsArgs<T> a;
  const NsPlan p = ns_plan<T>(N, D, nnz, L, &a, ws);
  GPZ_REQUIRE(ws_bytes >= p.bytes, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, p.bytes);
  a.c = c;
  a.W = static_cast<T*>(W);
  a.H = static_cast<T*>(H);
  return out ? ns_divergence_any<T>(a, out, s) : ns_iterate_any<T>(a, iters, s);
}

struct NsMatPlan { int64_t nchunks; size_t bytes; };

NsMatPlan ns_mat_plan(int64_t D, int64_t nnz, int k, int transpose, NsMatArgs* a, void* ws) {
  NsMatPlan p;
  p.nchunks = D + nnz / NS_CHUNK;
  Carver c(ws);
  int32_t* cstart = c.take<int32_t>(transpose ? (size_t)D + 1 : 1);
  int32_t* chunk_gene = c.take<int32_t>(transpose ? (size_t)p.nchunks : 1);
  double* part = c.take<double>(transpose ? (size_t)p.nchunks * k : 1);
  p.bytes = c.used();
  if (a) {
    a->cstart = cstart; a->chunk_gene = chunk_gene; a->part = part; a->nchunks = p.nchunks;
  }
  return p;
}

int ns_mat_check(const char* who, int64_t N, int64_t D, int64_t nnz, int k, int transpose) {
  GPZ_REQUIRE(k >= 1 && k <= NS_KMAX, "%s: k=%d unsupported (1..%d)", who, k, NS_KMAX);
  GPZ_REQUIRE(transpose == 0 || transpose == 1, "%s: transpose=%d (0: X Q, 1: X^T Q)", who, transpose);
  return ns_check_counts(who, N, D, nnz);
}

}  // namespace
}  // namespace gpz

using namespace gpz;

extern "C" int gpz_nmf_kl_sparse_plan(int64_t N, int64_t D, int64_t nnz, int32_t L, int32_t dtype, int32_t* spot_chunk,
                                      int32_t* gene_chunk, int64_t* n_gene_chunks, int32_t* factors_padded,
                                      int32_t* colsum_rows) {
  if (int rc = ns_check_shape("gpz_nmf_kl_sparse_plan", N, D, nnz, L, dtype)) return rc;
  if (spot_chunk) *spot_chunk = 0;
  if (gene_chunk) *gene_chunk = NS_CHUNK;
  if (n_gene_chunks) *n_gene_chunks = D + nnz / NS_CHUNK;
  if (factors_padded) *factors_padded = ns_instance(L);
  if (colsum_rows) *colsum_rows = NS_ROWS;
  return 0;
}

extern "C" size_t gpz_nmf_kl_sparse_workspace_bytes(int64_t N, int64_t D, int64_t nnz, int32_t L, int32_t dtype) {
  if (ns_check_shape("gpz_nmf_kl_sparse_workspace_bytes", N, D, nnz, L, dtype)) return 0;
  return ns_plan_bytes(N, D, nnz, L, dtype);
}

extern "C" int gpz_nmf_kl_sparse_update(const int64_t* col_ptr, const int32_t* col_gene, const float* col_val,
                                        const int64_t* row_ptr, const int32_t* row_spot, const int32_t* row_perm, void* W,
                                        void* H, int64_t N, int64_t D, int64_t nnz, int32_t L, int32_t dtype, int64_t iters,
                                        void* ws, size_t ws_bytes, void* stream) {
  const char* who = "gpz_nmf_kl_sparse_update";
  const NsCounts c{col_ptr, col_gene, col_val, row_ptr, row_spot, row_perm};
  if (int rc = ns_check_shape(who, N, D, nnz, L, dtype)) return rc;
  GPZ_REQUIRE(W && H, "%s: null pointer", who);
  if (int rc = ns_check_pointers(who, c, nnz, ws)) return rc;
  GPZ_REQUIRE(iters >= 1, "%s: iters=%lld unsupported (>= 1)", who, (long long)iters);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return dtype == GPZ_F32 ? ns_run<float>(who, c, W, H, N, D, nnz, L, iters, nullptr, ws, ws_bytes, s)
                          : ns_run<double>(who, c, W, H, N, D, nnz, L, iters, nullptr, ws, ws_bytes, s);
}

extern "C" int gpz_nmf_kl_sparse_divergence(const int64_t* col_ptr, const int32_t* col_gene, const float* col_val,
                                            const int64_t* row_ptr, const int32_t* row_spot, const int32_t* row_perm,
                                            const void* W, const void* H, int64_t N, int64_t D, int64_t nnz, int32_t L,
                                            int32_t dtype, double* out, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "gpz_nmf_kl_sparse_divergence";
  const NsCounts c{col_ptr, col_gene, col_val, row_ptr, row_spot, row_perm};
  if (int rc = ns_check_shape(who, N, D, nnz, L, dtype)) return rc;
  GPZ_REQUIRE(W && H && out, "%s: null pointer", who);
  if (int rc = ns_check_pointers(who, c, nnz, ws)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  void* Wm = const_cast<void*>(W);
  void* Hm = const_cast<void*>(H);
  return dtype == GPZ_F32 ? ns_run<float>(who, c, Wm, Hm, N, D, nnz, L, 0, out, ws, ws_bytes, s)
                          : ns_run<double>(who, c, Wm, Hm, N, D, nnz, L, 0, out, ws, ws_bytes, s);
}

extern "C" size_t gpz_counts_matmul_workspace_bytes(int64_t N, int64_t D, int64_t nnz, int32_t k, int32_t transpose) {
  if (ns_mat_check("gpz_counts_matmul_workspace_bytes", N, D, nnz, k, transpose)) return 0;
  return ns_mat_plan(D, nnz, k, transpose, nullptr, nullptr).bytes;
}

extern "C" int gpz_counts_matmul(const int64_t* col_ptr, const int32_t* col_gene, const float* col_val, const int64_t* row_ptr,
                                 const int32_t* row_spot, const int32_t* row_perm, const double* Q, double* out, int64_t N,
                                 int64_t D, int64_t nnz, int32_t k, int32_t transpose, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "gpz_counts_matmul";
  NsMatArgs a;
  a.c = NsCounts{col_ptr, col_gene, col_val, row_ptr, row_spot, row_perm};
  if (int rc = ns_mat_check(who, N, D, nnz, k, transpose)) return rc;
  GPZ_REQUIRE(Q && out, "%s: null pointer", who);
  if (int rc = ns_check_pointers(who, a.c, nnz, ws)) return rc;
  const NsMatPlan p = ns_mat_plan(D, nnz, k, transpose, &a, ws);
  GPZ_REQUIRE(ws_bytes >= p.bytes, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, p.bytes);
  a.Q = Q; a.out = out; a.N = N; a.D = D; a.nnz = nnz; a.k = k;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!transpose) {
    hipLaunchKernelGGL((ns_matmul_kernel<false>), dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, a);
    GPZ_LAUNCH_OK();
    return 0;
  }
  hipLaunchKernelGGL(chunks_kernel, dim3(1), dim3(1024), 0, s, row_ptr, D, a.nchunks, NS_CHUNK, false, a.cstart, a.chunk_gene);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL((ns_matmul_kernel<true>), dim3((unsigned)((a.nchunks + 3) / 4)), dim3(256), 0, s, a);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(ns_matmul_finish_kernel, dim3((unsigned)((D * k + 255) / 256)), dim3(256), 0, s, a);
  GPZ_LAUNCH_OK();
  return 0;
}
