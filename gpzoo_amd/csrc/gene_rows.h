// gene_rows.h -- what the per-gene kernels over a whole data set stored as its non-zeros share (gene_rank.hip,
// gene_dispersion.hip, spatial_stats.hip, moran_perm.hip): the by-gene arrays of gpzoo_amd.likelihoods.SparseCounts, the clamped row of a gene,
// the checked read of one stored entry, the fixed binary tree that closes a workgroup's partial sums, the row accessors of
// the Moran passes, and the check of the extents.
//
// Gene d owns [row_ptr[d], row_ptr[d + 1]), its k-th entry sits at spot row_spot[k] and has the value col_val[row_perm[k]].
// One workgroup of GR_THREADS threads works on one gene at a time; thread t adds the entries t, t + GR_THREADS, ... of the
// row in that order in fp64 and the GR_THREADS partial sums are added in a fixed binary tree: the result of a gene depends
// on neither the grid nor the workgroup that computes it.
#pragma once
#include "common.h"

namespace gpz {
namespace grk {

constexpr int GR_THREADS = 256;    // threads of a workgroup = stored entries of a row per sweep (the plan's gene_chunk)

struct GrRows {
  const int64_t* row_ptr; const int32_t* row_spot; const int32_t* row_perm; const float* col_val;
  int64_t N, D, nnz;
};

// red[0] = the sum of red[0 .. GR_THREADS) in a fixed binary tree; every thread of the workgroup calls it
template <int NV>
__device__ inline void gr_tree(double (*red)[GR_THREADS]) {
  __syncthreads();
  for (int h = GR_THREADS / 2; h >= 1; h >>= 1) {
    if (int(threadIdx.x) < h)
      for (int v = 0; v < NV; ++v) red[v][threadIdx.x] += red[v][threadIdx.x + h];
    __syncthreads();
  }
}

// the row of gene d, clamped to the stored entries: an inconsistent row_ptr reads nothing out of bounds
__device__ inline void gr_row(const GrRows& r, int64_t d, int64_t& lo, int64_t& hi) {
  lo = r.row_ptr[d];
  hi = r.row_ptr[d + 1];
  lo = lo < 0 ? 0 : (lo > r.nnz ? r.nnz : lo);
  hi = hi < lo ? lo : (hi > r.nnz ? r.nnz : hi);
}

__device__ inline bool gr_entry(const GrRows& r, int64_t k, int32_t& spot, float& x) {
  spot = r.row_spot[k];
  const int32_t p = r.row_perm[k];
  if (spot < 0 || spot >= r.N || p < 0 || p >= r.nnz) return false;
  x = r.col_val[p];
  return true;
}

// Row accessors of the Moran passes (moran_expr.h, moran_perm.hip): where the entries of gene d are and where a spot's value
// is looked up.  SparseRows: the stored entries, scattered into a line of N floats by the kernel (STAGED).  DenseRows: a
// contiguous fp32 (D, N) array, every spot an entry (zeros included), the row its own line.
struct SparseRows {
  static constexpr bool STAGED = true;
  GrRows r;
  __device__ int64_t spots() const { return r.N; }
  __device__ int64_t genes() const { return r.D; }
  __device__ void row(int64_t d, int64_t& lo, int64_t& hi) const { gr_row(r, d, lo, hi); }
  __device__ bool entry(int64_t, int64_t k, int32_t& spot, float& x) const { return gr_entry(r, k, spot, x); }
  __device__ bool spot_of(int64_t, int64_t k, int32_t& spot) const {
    spot = r.row_spot[k];
    return spot >= 0 && spot < r.N;
  }
  __device__ const float* line(int64_t) const { return nullptr; }
};

struct DenseRows {
  static constexpr bool STAGED = false;
  const float* v;
  int64_t N, D;
  __device__ int64_t spots() const { return N; }
  __device__ int64_t genes() const { return D; }
  __device__ void row(int64_t d, int64_t& lo, int64_t& hi) const {
    lo = d * N;
    hi = lo + N;
  }
  __device__ bool entry(int64_t lo, int64_t k, int32_t& spot, float& x) const {
    spot = int32_t(k - lo);
    x = v[k];
    return true;
  }
  __device__ bool spot_of(int64_t lo, int64_t k, int32_t& spot) const {
    spot = int32_t(k - lo);
    return true;
  }
  __device__ const float* line(int64_t d) const { return v + d * N; }
};

static int gr_check_shape(const char* who, int64_t N, int64_t D, int64_t nnz) {
  GPZ_REQUIRE(N >= 1 && D >= 1 && nnz >= 0, "%s: bad extents (N = %lld, D = %lld, nnz = %lld)", who, (long long)N, (long long)D,
              (long long)nnz);
  GPZ_REQUIRE(N < (1ll << 31) && D < (1ll << 31) && nnz < (1ll << 31), "%s: spots, genes and non-zeros are indexed with 32 bits",
              who);
  return 0;
}

}  // namespace grk
}  // namespace gpz
