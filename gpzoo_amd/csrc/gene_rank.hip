// gene_rank.hip -- two per-gene scores of counts (or log-normalised values) stored as their non-zeros, for ranking and
// selecting genes ahead of a fit: the deviance against a constant-rate null (scry's devianceFeatureSelection, the nsf
// paper's ranking) and Moran's I over the spots' K-neighbour graph (squidpy's spatial_autocorr(mode="moran")).  Both are
// exact sums over the stored entries plus O(N + D) terms; nothing of D x N or nnz elements is allocated.
//
// The data set arrives in the by-gene order of gpzoo_amd.likelihoods.SparseCounts: gene d owns [row_ptr[d], row_ptr[d + 1]),
// its k-th entry sits at spot row_spot[k] and has the value col_val[row_perm[k]].
//
// Deviance, S = sum_n size[n], sum = sum_nz y, p = sum / S:
//   Poisson   2 [ sum_nz y log(y / size_n) - sum log(sum / S) ]
//   binomial  2 [ sum_nz ( y log(y / size_n) + (size_n - y) log1p(-y / size_n) ) - sum (log p - log1p(-p)) - S log1p(-p) ]
// Moran's I with weights 1 / K, xbar = S / N, S = sum x, Q = sum x^2, C = sum_{i in nz} x_i sum_{j in nbr(i)} x_j,
// A = sum_{i in nz} indeg(i) x_i (sum_i sum_{j in nbr(i)} x_j with the two sums exchanged):
//   I = [ C - xbar (K S + A) + N K xbar^2 ] / ( K (Q - N xbar^2) )
// -- sum_i z_i sum_j z_j of the dense kernel (spatial.hip) expanded around the zeros, which are never visited.
//
// Gene pass (both entries; its helpers are gene_rows.h's, shared with gene_dispersion.hip): one workgroup of GR_THREADS
// threads per gene at a time, genes dealt to a fixed number of
// workgroups in a fixed order (gene d, d + G, ...).  Thread t adds the entries t, t + GR_THREADS, ... of the row in that
// order in fp64, the GR_THREADS partial sums are added in a fixed binary tree: the result of a gene depends on neither the
// grid nor the workgroup that computes it, and two calls agree bit for bit.  A row of N entries is GR_THREADS-wide
// coalesced sweeps; a row of one entry costs one sweep, and the other workgroups keep the device busy meanwhile.
//
// Neighbour lookup of the Moran pass: every workgroup owns one line of N floats in the scratch memory, which it zeroes
// itself at the start of the launch.  Per gene it scatters the row into the line, gathers the K neighbours of every stored
// entry from it, and then clears exactly the words it scattered: O(nnz (K + 2)) memory operations, no search, and a
// scratch of workgroups x N x 4 bytes whatever D is.  The in-degree of the table is counted once per call with integer
// atomics (a histogram; no atomics on values); that pass also checks every entry of the table and raises info.  The gene
// pass, its host driver and the closing expressions live in moran_expr.h, which spatial_stats.hip (Geary's C and the moments
// beside I: the same kernel, instantiated wide) and moran_perm.hip (the permutation null) include too.
//
// Built with -ffp-contract=off: every product and sum of the closing formulas is rounded on its own, so the numbers are
// those of the same expressions written in numpy (the CPU tests evaluate them that way), not of a compiler's choice of fma.
// The kernels wait for memory, not for the ALUs, so this costs nothing.
#include "gene_rows.h"
#include "moran_expr.h"

namespace gpz {
namespace grk {

constexpr int GR_DEV_WG = 2048;    // workgroups of the deviance pass (eight per CU, a full CU of waves; it has no lines)

// S = sum_n size[n]: one workgroup, strided per thread, then the tree
__global__ __launch_bounds__(GR_THREADS) void gr_total_kernel(const double* __restrict__ size, int64_t N, double* __restrict__ total) {
  __shared__ double red[1][GR_THREADS];
  double a = 0.0;
  for (int64_t n = threadIdx.x; n < N; n += GR_THREADS) a += size[n];
  red[0][threadIdx.x] = a;
  gr_tree<1>(red);
  if (threadIdx.x == 0) total[0] = red[0][0];
}

__global__ __launch_bounds__(GR_THREADS) void gr_deviance_kernel(GrRows r, const double* __restrict__ size, int family,
                                                                 const double* __restrict__ total, double* __restrict__ sum,
                                                                 double* __restrict__ count, double* __restrict__ deviance) {
  __shared__ double red[2][GR_THREADS];
  const double S = total[0];
  for (int64_t d = blockIdx.x; d < r.D; d += gridDim.x) {
    int64_t lo, hi;
    gr_row(r, d, lo, hi);
    double sy = 0.0, sat = 0.0;
    for (int64_t k = lo + threadIdx.x; k < hi; k += GR_THREADS) {
      int32_t spot;
      float x;
      if (!gr_entry(r, k, spot, x)) continue;
      const double y = double(x);
      sy += y;
      if (y > 0.0) {
        const double sz = size[spot], q = y / sz;
        double t = y * log(q);
        if (family == 1 && sz > y) t += (sz - y) * log1p(-q);      // y == size_n: y log 1 + 0
        sat += t;
      }
    }
    red[0][threadIdx.x] = sy;
    red[1][threadIdx.x] = sat;
    gr_tree<2>(red);
    if (threadIdx.x == 0) {
      const double s = red[0][0];
      double null = 0.0;
      if (s > 0.0) {
        const double p = s / S;
        if (family == 0) {
          null = s * log(p);
        } else if (p < 1.0) {
          const double l1 = log1p(-p);
          null = s * (log(p) - l1) + S * l1;
        }                                                           // p = 1: sum log 1 + 0
      }
      sum[d] = s;
      count[d] = double(hi - lo);
      deviance[d] = hi > lo ? 2.0 * (red[1][0] - null) : 0.0;
    }
    __syncthreads();
  }
}

struct GrPlan {        // the deviance pass; the Moran pass has GenePass of moran_expr.h
  double* total;      // S
  int workgroups;
  size_t bytes;
};

static GrPlan gr_plan(int64_t D, void* scratch) {
  Carver c(scratch);
  GrPlan p{};
  p.workgroups = int(D < GR_DEV_WG ? D : GR_DEV_WG);
  p.total = c.take<double>(1);
  p.bytes = c.used();
  return p;
}

}  // namespace grk
}  // namespace gpz

using namespace gpz;
using namespace gpz::grk;

extern "C" int gpz_gene_deviance_sparse_plan(int64_t N, int64_t D, int64_t nnz, int32_t* gene_chunk, int32_t* workgroups,
                                             int64_t* partials_bytes) {
  if (int rc = gr_check_shape("gpz_gene_deviance_sparse", N, D, nnz)) return rc;
  const GrPlan p = gr_plan(D, nullptr);
  if (gene_chunk) *gene_chunk = GR_THREADS;
  if (workgroups) *workgroups = p.workgroups;
  if (partials_bytes) *partials_bytes = int64_t(p.bytes);
  return 0;
}

extern "C" int gpz_gene_deviance_sparse(const int64_t* row_ptr, const int32_t* row_spot, const int32_t* row_perm,
                                        const float* col_val, const double* size, int64_t N, int64_t D, int64_t nnz,
                                        int32_t family, double* sum, double* count, double* deviance, void* partials,
                                        size_t partials_bytes, void* stream) {
  GPZ_REQUIRE(row_ptr && size && sum && count && deviance && partials, "gpz_gene_deviance_sparse: null pointer");
  if (int rc = gr_check_shape("gpz_gene_deviance_sparse", N, D, nnz)) return rc;
  GPZ_REQUIRE(nnz == 0 || (row_spot && row_perm && col_val), "gpz_gene_deviance_sparse: null pointer (non-zeros)");
  GPZ_REQUIRE(family == 0 || family == 1, "gpz_gene_deviance_sparse: family %d unknown (0 Poisson, 1 binomial)", family);
  GPZ_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 15) == 0, "gpz_gene_deviance_sparse: partials must be 16-byte aligned");
  const GrPlan p = gr_plan(D, partials);
  GPZ_REQUIRE(partials_bytes >= p.bytes, "gpz_gene_deviance_sparse: partials too small (%zu bytes, %zu needed)", partials_bytes,
              p.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const GrRows r{row_ptr, row_spot, row_perm, col_val, N, D, nnz};
  hipLaunchKernelGGL(gr_total_kernel, dim3(1), dim3(GR_THREADS), 0, s, size, N, p.total);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(gr_deviance_kernel, dim3(unsigned(p.workgroups)), dim3(GR_THREADS), 0, s, r, size, int(family), p.total, sum,
                     count, deviance);
  GPZ_LAUNCH_OK();
  return 0;
}

extern "C" int gpz_gene_morans_i_sparse_plan(int64_t N, int64_t D, int64_t nnz, int32_t K, int32_t* gene_chunk,
                                             int32_t* workgroups, int64_t* partials_bytes) {
  return gene_pass_query("gpz_gene_morans_i_sparse", N, D, nnz, K, gene_chunk, workgroups, partials_bytes);
}

extern "C" int gpz_gene_morans_i_sparse(const int64_t* row_ptr, const int32_t* row_spot, const int32_t* row_perm,
                                        const float* col_val, const int64_t* nbr, int64_t N, int64_t D, int64_t nnz, int32_t K,
                                        double* I, int32_t* info, void* partials, size_t partials_bytes, void* stream) {
  GPZ_REQUIRE(I, "gpz_gene_morans_i_sparse: null pointer");
  return gene_pass_entry<false>("gpz_gene_morans_i_sparse", GrRows{row_ptr, row_spot, row_perm, col_val, N, D, nnz}, nbr, K,
                                SsOut{I, nullptr, nullptr, nullptr, nullptr}, info, partials, partials_bytes, stream);
}
