// moran_pass.h -- the column pass of spatial_stats.hip over an fp32 slab, for callers inside the library (residual.hip):
// narrow (Moran's I), wide (Geary's C, the kurtosis beside it) and the permutation column pass, which scores the resident
// slab under relabelled neighbour tables.  The kernels are mi_rows / mi_final of spatial_stats.hip and their permutation
// siblings there, built with fp contraction off; gpz_morans_i and gpz_spatial_stats run the same ones.  The relabelled
// tables are written by mp_relabel_kernel of moran_perm.hip, reached through relabel_tables below.
#pragma once
#include "common.h"

namespace gpz {

// bytes of scratch for a slab of B rows and up to `cols` columns
size_t moran_slab_bytes(int64_t B, int64_t cols);

// Columns 0 .. cols of slab (B rows of ld floats each, cols <= ld) over nbr (B, K): I, the column mean and the column
// variance sum z^2 / B, cols fp64 values each.  info[0] is set to 1 by a table entry outside [0, B) or naming its own row
// (it is not cleared here).  Every sum in a fixed order.
int moran_slab_run(const float* slab, int64_t B, int64_t cols, int64_t ld, const int64_t* nbr, int K, double* I, double* mean,
                   double* var, int32_t* info, void* scratch, hipStream_t s);

// The wide sibling: I, Geary's C, the mean, the variance and the kurtosis m4 / m2^2 of the same columns, cols fp64 values
// each (I, mean and var have moran_slab_run's bits).  The chunks' partial sums stay in `scratch` for moran_slab_perm_run.
size_t moran_slab_wide_bytes(int64_t B, int64_t cols);
int moran_slab_wide_run(const float* slab, int64_t B, int64_t cols, int64_t ld, const int64_t* nbr, int K, double* I, double* C,
                        double* mean, double* var, double* kurtosis, int32_t* info, void* scratch, hipStream_t s);

// moran_perm.hip: T_pi[pi[i], m] = pi[nbr[i, m]] (int32, (pb, N, K)) for the pb rows of perms (pb, N); `written` (pb, N)
// is cleared here.  A row of perms that is no permutation sets info[0] = 2; a bad entry of nbr or perms becomes -1 in T.
// indeg (N,) -> indeg_pi (pb, N) where both are given (the gene entries); the column form needs neither.
int relabel_tables(const int64_t* nbr, const int32_t* indeg, const int32_t* perms, int64_t N, int K, int pb, int32_t* T,
                   int32_t* indeg_pi, int32_t* written, int32_t* info, hipStream_t s);

constexpr int SLAB_PERM_BATCH_MAX = 32;     // permutations per launch: the accumulators of one thread

// The permutation column pass.  After moran_slab_wide_run over the same slab, columns and nbr (wide_scratch is its scratch,
// mean its column means): the statistic (stat 0: I, 1: C) of every column under the P relabellings perms (P, B), in batches
// of perm_batch.  Per column, running over the permutations in order: n_ge / n_le (the numerator of the statistic >= / <=
// the observed one, in fp64), the mean of the simulated values and the sum of their squared deviations (Welford), which the
// caller has cleared before the first slab; sims (nullable) is the column's row of P values in an array whose rows are
// sims_ld apart.  Every sum fp64 in the order of mi_rows<TERMS = true> and mi_final, so the identity permutation gives the
// observed value bit for bit.  No floating-point atomics.
struct SlabPermOut {
  int32_t* n_ge;
  int32_t* n_le;
  double* sim_mean;
  double* sim_m2;
  double* sims;
  int64_t sims_ld;
  int32_t* info;
};
size_t moran_slab_perm_bytes(int64_t B, int64_t cols, int K, int perm_batch);
int moran_slab_perm_run(const float* slab, int64_t B, int64_t cols, int64_t ld, const int64_t* nbr, int K, int stat,
                        const int32_t* perms, int64_t P, int perm_batch, const double* mean, const void* wide_scratch,
                        const SlabPermOut& o, void* scratch, hipStream_t s);

}  // namespace gpz
