// moran_expr.h -- Moran's I, Geary's C and the moments of every gene from sums over its entries: the closing expressions, the
// in-degree pass, the gene pass and its host driver, shared by gene_rank.hip (gpz_gene_morans_i_sparse), spatial_stats.hip
// (gpz_gene_spatial_stats_sparse) and moran_perm.hip (the permutation entries).  All three are built with -ffp-contract=off:
// every product and sum below is rounded on its own, so they give the same bits from the same sums.
//
//   S = sum x, Q = sum x^2, C_s = sum_{i stored} x_i sum_{j in nbr(i)} x_j, A = sum_{i stored} indeg(i) x_i, xbar = S / N
//   I = [ C_s - xbar (K S + A) + N K xbar^2 ] / ( K (Q - N xbar^2) )
//
// A relabelling of the spots changes C_s and A only; the numerator is then C_s - S A / N, so N C_s - S A (moran_order) orders
// the statistic of one gene across relabellings -- exactly, for integer-valued data with |N C_s - S A| < 2^53.
//
// With binary weights over the table nbr (N, K), S0 = N K,
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

__device__ inline double geary_value(int64_t N, int K, double S, double Q, double Cs, double Qin, bool scored) {
  const double Nd = double(N), Kd = double(K);
  const double xbar = S / Nd;
  const double den = Kd * (Q - Nd * (xbar * xbar));                 // moran_value's
  const double G = Kd * Q + Qin - 2.0 * Cs;
  return (scored && den > 0.0) ? ((Nd - 1.0) * G) / (2.0 * Nd * den) : double(NAN);
}

__device__ inline double geary_order(double Cs, double Qin) { return Qin - 2.0 * Cs; }

struct SsOut {      // per gene, fp64 (D,); the narrow gene pass writes I alone, of the wide one each is nullable
  double* I;
  double* C;
  double* mean;
  double* var;
  double* kurtosis;
};

static int gr_check_k(const char* who, int64_t N, int32_t K) {
  GPZ_REQUIRE(K >= 1 && K <= GR_KMAX && K < N, "%s: K = %d neighbours of N = %lld spots unsupported (1 <= K <= %d, K < N)", who, K,
              (long long)N, GR_KMAX);
  return 0;
}

// every entry of the table once: the in-degree histogram (integer atomics) and the check of mi_rows (spatial_stats.hip) -- an entry outside
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

// The gene pass.  STAGED rows: every workgroup owns one line of N floats in `lines`, zeroes it at the start, scatters a
// gene's entries into it, gathers from it and clears what it scattered.  Otherwise the gene's row is the line.
// WIDE == false: the sums S, Q, C_s, A and o.I; `stats` (nullable, (D, GR_STATS)) keeps S, Q, moran_order and scored for the
// permutation kernels.  WIDE == true: one more sum (Q_in) beside them -- S, Q, C_s, A are added in the same order, so I has
// the same bits -- the second sweep where var or kurtosis is asked for, every field of o that is not null, and geary_order in
// the place of moran_order.
template <class Rows, bool WIDE>
__global__ __launch_bounds__(GR_THREADS) void gr_gene_kernel(Rows r, const int64_t* __restrict__ nbr, int K,
                                                             const int32_t* __restrict__ indeg, float* __restrict__ lines, SsOut o,
                                                             double* __restrict__ stats) {
  constexpr int SUMS = WIDE ? 5 : 4;
  __shared__ double red[SUMS][GR_THREADS];
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
      if constexpr (WIDE) qin += double(indeg[spot]) * (x * x);
      mn = xf < mn ? xf : mn;
      mx = xf > mx ? xf : mx;
    }
    red[0][threadIdx.x] = s;
    red[1][threadIdx.x] = q;
    red[2][threadIdx.x] = c;
    red[3][threadIdx.x] = a;
    if constexpr (WIDE) red[4][threadIdx.x] = qin;
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
        for (int v = 0; v < SUMS; ++v) red[v][threadIdx.x] += red[v][threadIdx.x + h];
        const float l2 = lohi[0][threadIdx.x + h], h2 = lohi[1][threadIdx.x + h];
        if (l2 < lohi[0][threadIdx.x]) lohi[0][threadIdx.x] = l2;
        if (h2 > lohi[1][threadIdx.x]) lohi[1][threadIdx.x] = h2;
      }
      __syncthreads();
    }
    const double S = red[0][0], Q = red[1][0], Cs = red[2][0], A = red[3][0], Qin = WIDE ? red[SUMS - 1][0] : 0.0;
    const bool scored = moran_scored(N, hi - lo, lohi[0][0], lohi[1][0]);
    const double xbar = S / double(N);
    bool sweep = false;
    if constexpr (WIDE) {
      sweep = o.var != nullptr || o.kurtosis != nullptr;           // the same for every thread
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
        __syncthreads();                                          // every thread has read the first sweep's sums
        red[0][threadIdx.x] = m2;
        red[1][threadIdx.x] = m4;
        gr_tree<2>(red);
      }
    }
    if (threadIdx.x == 0) {
      if (!WIDE || o.I) o.I[d] = moran_value(N, K, S, Q, Cs, A, scored);
      if constexpr (WIDE) {
        if (o.C) o.C[d] = geary_value(N, K, S, Q, Cs, Qin, scored);
        if (o.mean) o.mean[d] = xbar;
      }
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
        stats[d * GR_STATS + 2] = WIDE ? geary_order(Cs, Qin) : moran_order(N, S, Cs, A);
        stats[d * GR_STATS + 3] = scored ? 1.0 : 0.0;
      }
    }
    __syncthreads();                                              // the line is clear and red is free for the next gene
  }
}

// The host side of the gene pass: its share of the scratch memory (carved first: a caller's own arrays follow it), and
// "clear info and the in-degrees, count them, run the gene kernel".  staged = rows stored as their non-zeros.
struct GenePass {
  int32_t* indeg;     // (N,)
  float* lines;       // (workgroups, N): staged rows only
  int workgroups;

  GenePass(Carver& c, int64_t N, int64_t D, bool staged) : lines(nullptr), workgroups(int(D < GR_MAX_WG ? D : GR_MAX_WG)) {
    indeg = c.take<int32_t>(size_t(N));
    if (staged) lines = c.take<float>(size_t(workgroups) * size_t(N));
  }

  template <bool WIDE, class Rows>
  int run(const Rows& r, const int64_t* nbr, int64_t N, int K, const SsOut& o, double* stats, int32_t* info, hipStream_t s) const {
    GPZ_HIP_OK(hipMemsetAsync(info, 0, sizeof(int32_t), s));
    GPZ_HIP_OK(hipMemsetAsync(indeg, 0, size_t(N) * sizeof(int32_t), s));
    hipLaunchKernelGGL(gr_indeg_kernel, dim3(unsigned((N * K + GR_THREADS - 1) / GR_THREADS)), dim3(GR_THREADS), 0, s, nbr, N, K, indeg,
                       info);
    GPZ_LAUNCH_OK();
    hipLaunchKernelGGL((gr_gene_kernel<Rows, WIDE>), dim3(unsigned(workgroups)), dim3(GR_THREADS), 0, s, r, nbr, K, indeg, lines, o, stats);
    GPZ_LAUNCH_OK();
    return 0;
  }
};

// What gpz_gene_morans_i_sparse (WIDE == false) and gpz_gene_spatial_stats_sparse (true) share beyond their outputs: the plan
// query, and the entry after its own check of the output pointers.
static int gene_pass_query(const char* who, int64_t N, int64_t D, int64_t nnz, int32_t K, int32_t* gene_chunk, int32_t* workgroups,
                           int64_t* partials_bytes) {
  if (int rc = gr_check_shape(who, N, D, nnz)) return rc;
  if (int rc = gr_check_k(who, N, K)) return rc;
  Carver c(nullptr);
  const GenePass p(c, N, D, true);
  if (gene_chunk) *gene_chunk = GR_THREADS;
  if (workgroups) *workgroups = p.workgroups;
  if (partials_bytes) *partials_bytes = int64_t(c.used());
  return 0;
}

template <bool WIDE>
static int gene_pass_entry(const char* who, const GrRows& r, const int64_t* nbr, int32_t K, const SsOut& o, int32_t* info, void* partials,
                           size_t partials_bytes, void* stream) {
  GPZ_REQUIRE(r.row_ptr && nbr && info && partials, "%s: null pointer", who);
  if (int rc = gr_check_shape(who, r.N, r.D, r.nnz)) return rc;
  if (int rc = gr_check_k(who, r.N, K)) return rc;
  GPZ_REQUIRE(r.nnz == 0 || (r.row_spot && r.row_perm && r.col_val), "%s: null pointer (non-zeros)", who);
  GPZ_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 15) == 0, "%s: partials must be 16-byte aligned", who);
  Carver c(partials);
  const GenePass p(c, r.N, r.D, true);
  GPZ_REQUIRE(partials_bytes >= c.used(), "%s: partials too small (%zu bytes, %zu needed)", who, partials_bytes, c.used());
  return p.run<WIDE>(SparseRows{r}, nbr, r.N, int(K), o, nullptr, info, static_cast<hipStream_t>(stream));
}

}  // namespace grk
}  // namespace gpz
