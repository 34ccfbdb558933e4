// moran_expr.h -- Moran's I of every gene from sums over its entries: the closing expression, the in-degree pass and the
// gene pass, shared by gene_rank.hip (gpz_gene_morans_i_sparse) and moran_perm.hip (the permutation entries).  Both files
// are built with -ffp-contract=off: every product and sum below is rounded on its own, so the two give the same bits from
// the same sums.
//
//   S = sum x, Q = sum x^2, C = sum_{i stored} x_i sum_{j in nbr(i)} x_j, A = sum_{i stored} indeg(i) x_i, xbar = S / N
//   I = [ C - xbar (K S + A) + N K xbar^2 ] / ( K (Q - N xbar^2) )
//
// A relabelling of the spots changes C and A only; the numerator is then C - S A / N, so N C - S A (moran_order) orders the
// statistic of one gene across relabellings -- exactly, for integer-valued data with |N C - S A| < 2^53.
#pragma once
#include "gene_rows.h"

namespace gpz {
namespace grk {

constexpr int GR_MAX_WG = 256;     // workgroups of the Moran pass (one per CU): its scratch is GR_MAX_WG lines, and more lines
                                   // in flight bought nothing (measured: DESIGN.md section 5)
constexpr int GR_KMAX = 32;
constexpr int GR_STATS = 4;        // per gene, for the permutation entries: S, Q, N C - S A, scored (1 or 0)

// a gene scores at all: it has entries and is not stored at every spot with one single value (found from count, min and
// max, not from the cancelled denominator)
__device__ inline bool moran_scored(int64_t N, int64_t stored, float mn, float mx) {
  const bool constant = stored == N && mn == mx;
  return stored > 0 && !constant;
}

__device__ inline double moran_value(int64_t N, int K, double S, double Q, double Cs, double A, bool scored) {
  const double Nd = double(N), Kd = double(K);
  const double xbar = S / Nd;
  const double den = Kd * (Q - Nd * (xbar * xbar));
  const double num = Cs - xbar * (Kd * S + A) + Nd * Kd * (xbar * xbar);
  return (scored && den > 0.0) ? num / den : double(NAN);
}

__device__ inline double moran_order(int64_t N, double S, double Cs, double A) { return double(N) * Cs - S * A; }

static int gr_check_k(const char* who, int64_t N, int32_t K) {
  GPZ_REQUIRE(K >= 1 && K <= GR_KMAX && K < N, "%s: K = %d neighbours of N = %lld spots unsupported (1 <= K <= %d, K < N)", who, K,
              (long long)N, GR_KMAX);
  return 0;
}

// every entry of the table once: the in-degree histogram (integer atomics) and the check of mi_rows -- an entry outside
// [0, N) or naming its own row is counted nowhere, read nowhere, and raises info
static __global__ __launch_bounds__(GR_THREADS) void gr_indeg_kernel(const int64_t* __restrict__ nbr, int64_t N, int K,
                                                                     int32_t* __restrict__ indeg, int32_t* __restrict__ info) {
  const int64_t e = int64_t(blockIdx.x) * GR_THREADS + threadIdx.x;
  if (e >= N * K) return;
  const int64_t i = e / K, j = nbr[e];
  if (j < 0 || j >= N || j == i) {
    *info = 1;
    return;
  }
  atomicAdd(indeg + j, 1);
}

// I of every gene.  STAGED rows: every workgroup owns one line of N floats in `lines`, zeroes it at the start, scatters a
// gene's entries into it, gathers from it and clears what it scattered.  Otherwise the gene's row is the line.  `stats`
// (nullable, (D, GR_STATS)) keeps what the permutation kernels need of the gene.
template <class Rows>
__global__ __launch_bounds__(GR_THREADS) void gr_moran_kernel(Rows r, const int64_t* __restrict__ nbr, int K,
                                                              const int32_t* __restrict__ indeg, float* __restrict__ lines,
                                                              double* __restrict__ I, double* __restrict__ stats) {
  __shared__ double red[4][GR_THREADS];
  __shared__ float lohi[2][GR_THREADS];
  const int64_t N = r.spots();
  float* staged = nullptr;
  if constexpr (Rows::STAGED) {
    staged = lines + int64_t(blockIdx.x) * N;
    for (int64_t n = threadIdx.x; n < N; n += GR_THREADS) staged[n] = 0.0f;
    __syncthreads();
  }
  for (int64_t d = blockIdx.x; d < r.genes(); d += gridDim.x) {
    int64_t lo, hi;
    r.row(d, lo, hi);
    const float* line = Rows::STAGED ? staged : r.line(d);
    if constexpr (Rows::STAGED) {
      for (int64_t k = lo + threadIdx.x; k < hi; k += GR_THREADS) {
        int32_t spot;
        float x;
        if (r.entry(lo, k, spot, x)) staged[spot] = x;
      }
      __syncthreads();
    }
    double s = 0.0, q = 0.0, c = 0.0, a = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    for (int64_t k = lo + threadIdx.x; k < hi; k += GR_THREADS) {
      int32_t spot;
      float xf;
      if (!r.entry(lo, k, spot, xf)) continue;
      const double x = double(xf);
      const int64_t* __restrict__ row = nbr + int64_t(spot) * K;
      double lag = 0.0;
      for (int m = 0; m < K; ++m) {
        const int64_t j = row[m];
        if (j < 0 || j >= N || j == spot) continue;              // gr_indeg_kernel has told the caller
        lag += double(line[j]);
      }
      s += x;
      q += x * x;
      c += x * lag;
      a += double(indeg[spot]) * x;
      mn = xf < mn ? xf : mn;
      mx = xf > mx ? xf : mx;
    }
    red[0][threadIdx.x] = s;
    red[1][threadIdx.x] = q;
    red[2][threadIdx.x] = c;
    red[3][threadIdx.x] = a;
    lohi[0][threadIdx.x] = mn;
    lohi[1][threadIdx.x] = mx;
    __syncthreads();                                              // every gather of the line is done
    if constexpr (Rows::STAGED) {
      for (int64_t k = lo + threadIdx.x; k < hi; k += GR_THREADS) {
        int32_t spot;
        if (r.spot_of(lo, k, spot)) staged[spot] = 0.0f;
      }
    }
    for (int h = GR_THREADS / 2; h >= 1; h >>= 1) {
      if (int(threadIdx.x) < h) {
        for (int v = 0; v < 4; ++v) red[v][threadIdx.x] += red[v][threadIdx.x + h];
        const float l2 = lohi[0][threadIdx.x + h], h2 = lohi[1][threadIdx.x + h];
        if (l2 < lohi[0][threadIdx.x]) lohi[0][threadIdx.x] = l2;
        if (h2 > lohi[1][threadIdx.x]) lohi[1][threadIdx.x] = h2;
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      const bool scored = moran_scored(N, hi - lo, lohi[0][0], lohi[1][0]);
      I[d] = moran_value(N, K, red[0][0], red[1][0], red[2][0], red[3][0], scored);
      if (stats) {
        stats[d * GR_STATS + 0] = red[0][0];
        stats[d * GR_STATS + 1] = red[1][0];
        stats[d * GR_STATS + 2] = moran_order(N, red[0][0], red[2][0], red[3][0]);
        stats[d * GR_STATS + 3] = scored ? 1.0 : 0.0;
      }
    }
    __syncthreads();                                              // the line is clear and red is free for the next gene
  }
}

}  // namespace grk
}  // namespace gpz
