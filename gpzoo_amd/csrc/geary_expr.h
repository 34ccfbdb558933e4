// geary_expr.h -- Geary's C and the moments of every gene from sums over its entries, next to Moran's I of moran_expr.h: the
// closing expression and the gene pass, shared by spatial_stats.hip (gpz_gene_spatial_stats_sparse) and the permutation
// kernels of moran_perm.h.  Built with -ffp-contract=off like everything that includes moran_expr.h.
//
// With binary weights over the table nbr (N, K), S0 = N K and the sums S, Q, C_s, A of moran_expr.h,
//   G = sum_i sum_{j in nbr(i)} (x_i - x_j)^2 = K Q + Q_in - 2 C_s,   Q_in = sum_{i stored} indeg(i) x_i^2,
//   C = (N - 1) G / ( 2 N K (Q - N xbar^2) ).
// G does not change when a constant is added to every spot.  A relabelling of the spots changes Q_in and C_s only, so
// Q_in - 2 C_s (geary_order) orders the statistic of one gene across relabellings -- exactly, for integer-valued data
// below 2^53.  The denominator is Moran's; a nearly constant gene loses digits in proportion to mean^2 / variance, in G as in
// the denominator.
//
// The central moments come from a second sweep of the row once xbar = S / N is known: m_k = [ sum_{stored} (x - xbar)^k +
// (N - stored) xbar^k ] / N for k = 2, 4 -- sums of non-negative terms, no cancellation -- and the kurtosis is b2 = m4 / m2^2.
#pragma once
#include "moran_expr.h"

namespace gpz {
namespace grk {

__device__ inline double geary_value(int64_t N, int K, double S, double Q, double Cs, double Qin, bool scored) {
  const double Nd = double(N), Kd = double(K);
  const double xbar = S / Nd;
  const double den = Kd * (Q - Nd * (xbar * xbar));                 // moran_value's
  const double G = Kd * Q + Qin - 2.0 * Cs;
  return (scored && den > 0.0) ? ((Nd - 1.0) * G) / (2.0 * Nd * den) : double(NAN);
}

__device__ inline double geary_order(double Cs, double Qin) { return Qin - 2.0 * Cs; }

struct SsOut {      // per gene, fp64 (D,), each nullable
  double* I;
  double* C;
  double* mean;
  double* var;
  double* kurtosis;
};

// gr_moran_kernel with one more sum (Q_in) and the second sweep: the sums S, Q, C_s, A are added in its order, so I has
// its bits.  `stats` (nullable, (D, GR_STATS)) keeps S, Q, Q_in - 2 C_s and scored for the permutation kernels.
template <class Rows>
__global__ __launch_bounds__(GR_THREADS) void ss_gene_kernel(Rows r, const int64_t* __restrict__ nbr, int K,
                                                             const int32_t* __restrict__ indeg, float* __restrict__ lines, SsOut o,
                                                             double* __restrict__ stats) {
  __shared__ double red[5][GR_THREADS];
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
    double s = 0.0, q = 0.0, c = 0.0, a = 0.0, qin = 0.0;
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
      qin += double(indeg[spot]) * (x * x);
      mn = xf < mn ? xf : mn;
      mx = xf > mx ? xf : mx;
    }
    red[0][threadIdx.x] = s;
    red[1][threadIdx.x] = q;
    red[2][threadIdx.x] = c;
    red[3][threadIdx.x] = a;
    red[4][threadIdx.x] = qin;
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
        for (int v = 0; v < 5; ++v) red[v][threadIdx.x] += red[v][threadIdx.x + h];
        const float l2 = lohi[0][threadIdx.x + h], h2 = lohi[1][threadIdx.x + h];
        if (l2 < lohi[0][threadIdx.x]) lohi[0][threadIdx.x] = l2;
        if (h2 > lohi[1][threadIdx.x]) lohi[1][threadIdx.x] = h2;
      }
      __syncthreads();
    }
    const double S = red[0][0], Q = red[1][0], Cs = red[2][0], A = red[3][0], Qin = red[4][0];
    const bool scored = moran_scored(N, hi - lo, lohi[0][0], lohi[1][0]);
    const double xbar = S / double(N);
    const bool sweep = o.var != nullptr || o.kurtosis != nullptr;   // the same for every thread
    if (sweep) {
      double m2 = 0.0, m4 = 0.0;
      for (int64_t k = lo + threadIdx.x; k < hi; k += GR_THREADS) {
        int32_t spot;
        float xf;
        if (!r.entry(lo, k, spot, xf)) continue;
        const double dx = double(xf) - xbar, d2 = dx * dx;
        m2 += d2;
        m4 += d2 * d2;
      }
      __syncthreads();                                            // every thread has read the first sweep's sums
      red[0][threadIdx.x] = m2;
      red[1][threadIdx.x] = m4;
      gr_tree<2>(red);
    }
    if (threadIdx.x == 0) {
      if (o.I) o.I[d] = moran_value(N, K, S, Q, Cs, A, scored);
      if (o.C) o.C[d] = geary_value(N, K, S, Q, Cs, Qin, scored);
      if (o.mean) o.mean[d] = xbar;
      if (sweep) {
        const int64_t rest = N - (hi - lo) > 0 ? N - (hi - lo) : 0;         // the spots without an entry: (0 - xbar)^k each
        const double x2 = xbar * xbar;
        const double m2 = (red[0][0] + double(rest) * x2) / double(N), m4 = (red[1][0] + double(rest) * (x2 * x2)) / double(N);
        if (o.var) o.var[d] = m2;
        if (o.kurtosis) o.kurtosis[d] = (scored && m2 > 0.0) ? m4 / (m2 * m2) : double(NAN);
      }
      if (stats) {
        stats[d * GR_STATS + 0] = S;
        stats[d * GR_STATS + 1] = Q;
        stats[d * GR_STATS + 2] = geary_order(Cs, Qin);
        stats[d * GR_STATS + 3] = scored ? 1.0 : 0.0;
      }
    }
    __syncthreads();                                              // the line is clear and red is free for the next gene
  }
}

}  // namespace grk
}  // namespace gpz
