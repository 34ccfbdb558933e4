// moran_perm.h -- the drivers of the permutation kernels (moran_perm.hip), for the entries that take the statistic as an
// argument (spatial_stats.hip).  The kernels are instantiated once, in moran_perm.hip, for both statistics.
#pragma once
#include "geary_expr.h"

namespace gpz {
namespace grk {

constexpr int STAT_MORAN = 0, STAT_GEARY = 1;

struct MpOut {
  double* I;          // the observed statistic: I, or C
  double* sims;
  int32_t* n_ge;
  int32_t* n_le;
  double* sim_mean;
  double* sim_m2;
  int32_t* info;
};

// the plan of a shape (host only; any out pointer may be NULL); staged = rows stored as their non-zeros
int mp_plan_query(const char* who, int64_t N, int64_t D, int32_t K, int64_t P, int32_t perm_batch_wanted, int32_t line_mode_wanted,
                  bool staged, int32_t* perm_batch, int32_t* line_mode, int32_t* workgroups, int64_t* partials_bytes);

// the statistic `stat` of every gene and of its P relabellings; the arguments are checked by the caller, except for what
// the plan checks (K, P, perm_batch, line_mode) and the scratch memory
int mp_run_sparse(const char* who, int stat, const GrRows& rows, const int64_t* nbr, const int32_t* perms, int32_t K, int64_t P,
                  int32_t perm_batch, int32_t line_mode, const MpOut& o, void* partials, size_t partials_bytes, void* stream);
int mp_run_rows(const char* who, int stat, const float* values, int64_t N, int64_t D, const int64_t* nbr, const int32_t* perms, int32_t K,
                int64_t P, int32_t perm_batch, int32_t line_mode, const MpOut& o, void* partials, size_t partials_bytes, void* stream);

}  // namespace grk
}  // namespace gpz
