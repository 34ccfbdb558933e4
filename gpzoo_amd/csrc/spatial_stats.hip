// spatial_stats.hip -- Moran's I, Geary's C, the mean, the variance and the kurtosis of every gene in one call, and the
// permutation null of either statistic: squidpy's spatial_autocorr(mode="moran" | "geary") / PySAL's Moran and Geary with what
// their randomisation moments (VI_rand, VC_rand) need of each gene, b2 = m4 / m2^2.
//
//   gpz_gene_spatial_stats_sparse   the by-gene arrays of a whole data set stored as its non-zeros: ss_gene_kernel of
//                                   geary_expr.h, one workgroup per gene at a time over the line handling of gr_moran_kernel.
//                                   I has gpz_gene_morans_i_sparse's bits.
//   gpz_spatial_stats               the first L columns of an (N, L) array, as gpz_morans_i takes them, in the arithmetic of
//                                   spatial.hip's mi_rows / mi_final (which this file repeats with two more sums, so that I has
//                                   gpz_morans_i's bits): the column sums shifted by the column's first value give the mean,
//                                   then per chunk of 256 rows sum z lag / K, sum z^2, sum_i sum_j (z_i - z_j)^2 and sum z^4
//                                   of z = v - mean, closed per column in a fixed order.  G is a sum of non-negative terms.
//   gpz_gene_autocorr_perm_sparse, gpz_autocorr_perm_rows   the permutation entries of moran_perm.hip with the statistic as
//                                   an argument, through its drivers (moran_perm.h).
// Built with -ffp-contract=off: every product and sum is rounded on its own, as in gene_rank.hip, moran_perm.hip and
// spatial.hip, whose bits these entries have to give.  No floating-point atomics; every sum fp64 in a fixed order.
#include "moran_perm.h"

namespace gpz {
namespace grk {

struct SsPlan {
  int32_t* indeg;     // (N,)
  float* lines;       // (workgroups, N)
  int workgroups;
  size_t bytes;
};

static SsPlan ss_plan(int64_t N, int64_t D, void* scratch) {
  Carver c(scratch);
  SsPlan p{};
  p.workgroups = int(D < GR_MAX_WG ? D : GR_MAX_WG);
  p.indeg = c.take<int32_t>(size_t(N));
  p.lines = c.take<float>(size_t(p.workgroups) * size_t(N));
  p.bytes = c.used();
  return p;
}

// ---- the columns of a dense array ----------------------------------------------------------------------------------------

constexpr int SC_THREADS = 256;
constexpr int SC_ROWS = 256;         // rows per partial sum, as spatial.hip's MI_ROWS
constexpr int SC_PART = 5;           // per (chunk, column): shifted sum, sum z lag / K, sum z^2, G, sum z^4

static int sc_cw(int64_t L) {        // threads of a block: cw columns x (SC_THREADS / cw) row slots
  int cw = 1;
  while (cw < L && cw < 64) cw <<= 1;
  return cw;
}

struct ScPlan {
  double* part;       // (chunks, L, SC_PART)
  double* mean;       // (L,)
  int64_t chunks;
  size_t bytes;
};

static ScPlan sc_plan(int64_t N, int64_t L, void* scratch) {
  Carver c(scratch);
  ScPlan p{};
  p.chunks = (N + SC_ROWS - 1) / SC_ROWS;
  p.part = c.take<double>(size_t(p.chunks) * size_t(L) * SC_PART);
  p.mean = c.take<double>(size_t(L));
  p.bytes = c.used();
  return p;
}

// Block (chunk, column tile): each thread sums its rows in order, then row slot 0 adds the slots in order.
template <typename T, bool TERMS>
__global__ __launch_bounds__(SC_THREADS) void sc_rows(const T* __restrict__ V, int64_t N, int64_t L, int cw,
                                                      const int64_t* __restrict__ nbr, int K, const double* __restrict__ mean,
                                                      double* __restrict__ part, int32_t* __restrict__ info) {
  __shared__ double red[4][SC_THREADS];
  const int c = threadIdx.x % cw, slot = threadIdx.x / cw, slots = SC_THREADS / cw;
  const int64_t l = int64_t(blockIdx.y) * cw + c;
  const int64_t r0 = int64_t(blockIdx.x) * SC_ROWS, r1 = r0 + SC_ROWS < N ? r0 + SC_ROWS : N;
  double a = 0.0, b = 0.0, g = 0.0, f = 0.0;
  if (l < L) {
    const double ref = TERMS ? mean[l] : double(V[l]);
    const double w = 1.0 / K;
    for (int64_t i = r0 + slot; i < r1; i += slots) {
      const double z = double(V[i * L + l]) - ref;
      if (!TERMS) {
        a += z;
        continue;
      }
      double lag = 0.0, gi = 0.0;
      for (int k = 0; k < K; ++k) {
        const int64_t j = nbr[i * K + k];
        if (j < 0 || j >= N || j == i) {     // never read outside the values; the caller is told through info
          *info = 1;
          continue;
        }
        const double zj = double(V[j * L + l]) - ref, dz = z - zj;
        lag += zj;
        gi += dz * dz;
      }
      const double z2 = z * z;
      a += z * (lag * w);
      b += z2;
      g += gi;
      f += z2 * z2;
    }
  }
  red[0][threadIdx.x] = a;
  red[1][threadIdx.x] = b;
  red[2][threadIdx.x] = g;
  red[3][threadIdx.x] = f;
  __syncthreads();
  if (slot == 0 && l < L) {
    for (int r = 1; r < slots; ++r) {
      a += red[0][r * cw + c];
      b += red[1][r * cw + c];
      g += red[2][r * cw + c];
      f += red[3][r * cw + c];
    }
    double* o = part + (int64_t(blockIdx.x) * L + l) * SC_PART;
    if (TERMS) {
      o[1] = a;
      o[2] = b;
      o[3] = g;
      o[4] = f;
    } else {
      o[0] = a;
    }
  }
}

// Block = column: the chunks' partials in a fixed order (strided per thread, then a fixed tree).  TERMS == false: the mean
// (first value + shifted sum / N) into the scratch memory and, where asked for, the output; TERMS == true: the rest.
template <typename T, bool TERMS>
__global__ __launch_bounds__(SC_THREADS) void sc_final(const double* __restrict__ part, int64_t chunks, int64_t L, int64_t N, int K,
                                                       const T* __restrict__ V, double* __restrict__ mean, SsOut o) {
  __shared__ double red[4][SC_THREADS];
  const int64_t l = blockIdx.x;
  double a = 0.0, b = 0.0, g = 0.0, f = 0.0;
  for (int64_t ch = threadIdx.x; ch < chunks; ch += SC_THREADS) {
    const double* p = part + (ch * L + l) * SC_PART;
    if (TERMS) {
      a += p[1];
      b += p[2];
      g += p[3];
      f += p[4];
    } else {
      a += p[0];
    }
  }
  red[0][threadIdx.x] = a;
  red[1][threadIdx.x] = b;
  red[2][threadIdx.x] = g;
  red[3][threadIdx.x] = f;
  __syncthreads();
  for (int h = SC_THREADS / 2; h >= 1; h >>= 1) {
    if (int(threadIdx.x) < h)
      for (int v = 0; v < 4; ++v) red[v][threadIdx.x] += red[v][threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  if (!TERMS) {
    const double m = double(V[l]) + red[0][0] / double(N);
    mean[l] = m;
    if (o.mean) o.mean[l] = m;
    return;
  }
  const double Nd = double(N), den = red[1][0], var = den / Nd;          // 0 / 0 = NaN: a constant column
  if (o.I) o.I[l] = red[0][0] / den;
  if (o.C) o.C[l] = ((Nd - 1.0) * red[2][0]) / (2.0 * Nd * double(K) * den);
  if (o.var) o.var[l] = var;
  if (o.kurtosis) o.kurtosis[l] = (red[3][0] / Nd) / (var * var);
}

template <typename T>
static int sc_run(const void* values, int64_t N, int64_t L, const int64_t* nbr, int K, const SsOut& o, int32_t* info, const ScPlan& pl,
                  hipStream_t s) {
  const T* V = static_cast<const T*>(values);
  const int cw = sc_cw(L);
  const dim3 rows(unsigned(pl.chunks), unsigned((L + cw - 1) / cw)), block(SC_THREADS);
  hipLaunchKernelGGL((sc_rows<T, false>), rows, block, 0, s, V, N, L, cw, nbr, K, pl.mean, pl.part, info);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL((sc_final<T, false>), dim3(unsigned(L)), block, 0, s, pl.part, pl.chunks, L, N, K, V, pl.mean, o);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL((sc_rows<T, true>), rows, block, 0, s, V, N, L, cw, nbr, K, pl.mean, pl.part, info);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL((sc_final<T, true>), dim3(unsigned(L)), block, 0, s, pl.part, pl.chunks, L, N, K, V, pl.mean, o);
  GPZ_LAUNCH_OK();
  return 0;
}

static int sc_check_args(const char* who, int64_t N, int64_t L, int32_t K, int32_t dtype) {
  GPZ_REQUIRE(dtype == GPZ_F32 || dtype == GPZ_F64, "%s: unknown dtype %d", who, dtype);
  GPZ_REQUIRE(K >= 1 && N > K && N < (int64_t(1) << 31), "%s: N=%lld, K=%d unsupported (1 <= K < N < 2^31)", who, (long long)N, K);
  GPZ_REQUIRE(L >= 1 && L <= (int64_t(1) << 20), "%s: L=%lld unsupported (1..2^20)", who, (long long)L);
  return 0;
}

static int ap_check_stat(const char* who, int32_t stat) {
  GPZ_REQUIRE(stat == STAT_MORAN || stat == STAT_GEARY, "%s: stat %d unknown (0 Moran's I, 1 Geary's C)", who, stat);
  return 0;
}

}  // namespace grk
}  // namespace gpz

using namespace gpz;
using namespace gpz::grk;

extern "C" int gpz_gene_spatial_stats_sparse_plan(int64_t N, int64_t D, int64_t nnz, int32_t K, int32_t* gene_chunk,
                                                  int32_t* workgroups, int64_t* partials_bytes) {
  if (int rc = gr_check_shape("gpz_gene_spatial_stats_sparse", N, D, nnz)) return rc;
  if (int rc = gr_check_k("gpz_gene_spatial_stats_sparse", N, K)) return rc;
  const SsPlan p = ss_plan(N, D, nullptr);
  if (gene_chunk) *gene_chunk = GR_THREADS;
  if (workgroups) *workgroups = p.workgroups;
  if (partials_bytes) *partials_bytes = int64_t(p.bytes);
  return 0;
}

extern "C" int gpz_gene_spatial_stats_sparse(const int64_t* row_ptr, const int32_t* row_spot, const int32_t* row_perm,
                                             const float* col_val, const int64_t* nbr, int64_t N, int64_t D, int64_t nnz, int32_t K,
                                             double* I, double* C, double* mean, double* var, double* kurtosis, int32_t* info,
                                             void* partials, size_t partials_bytes, void* stream) {
  const char* who = "gpz_gene_spatial_stats_sparse";
  GPZ_REQUIRE(row_ptr && nbr && info && partials, "%s: null pointer", who);
  if (int rc = gr_check_shape(who, N, D, nnz)) return rc;
  if (int rc = gr_check_k(who, N, K)) return rc;
  GPZ_REQUIRE(nnz == 0 || (row_spot && row_perm && col_val), "%s: null pointer (non-zeros)", who);
  GPZ_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 15) == 0, "%s: partials must be 16-byte aligned", who);
  const SsPlan p = ss_plan(N, D, partials);
  GPZ_REQUIRE(partials_bytes >= p.bytes, "%s: partials too small (%zu bytes, %zu needed)", who, partials_bytes, p.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const GrRows r{row_ptr, row_spot, row_perm, col_val, N, D, nnz};
  GPZ_HIP_OK(hipMemsetAsync(info, 0, sizeof(int32_t), s));
  GPZ_HIP_OK(hipMemsetAsync(p.indeg, 0, size_t(N) * sizeof(int32_t), s));
  hipLaunchKernelGGL(gr_indeg_kernel, dim3(unsigned((N * K + GR_THREADS - 1) / GR_THREADS)), dim3(GR_THREADS), 0, s, nbr, N, int(K),
                     p.indeg, info);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(ss_gene_kernel<SparseRows>, dim3(unsigned(p.workgroups)), dim3(GR_THREADS), 0, s, SparseRows{r}, nbr, int(K), p.indeg,
                     p.lines, SsOut{I, C, mean, var, kurtosis}, static_cast<double*>(nullptr));
  GPZ_LAUNCH_OK();
  return 0;
}

extern "C" int gpz_spatial_stats_plan(int64_t N, int64_t L, int32_t K, int32_t* row_chunk, int64_t* chunks, int64_t* partials_bytes) {
  if (int rc = sc_check_args("gpz_spatial_stats", N, L, K, GPZ_F64)) return rc;
  const ScPlan p = sc_plan(N, L, nullptr);
  if (row_chunk) *row_chunk = SC_ROWS;
  if (chunks) *chunks = p.chunks;
  if (partials_bytes) *partials_bytes = int64_t(p.bytes);
  return 0;
}

extern "C" int gpz_spatial_stats(const void* values, int64_t N, int64_t L, int32_t dtype, const int64_t* nbr, int32_t K, double* I,
                                 double* C, double* mean, double* var, double* kurtosis, int32_t* info, void* partials,
                                 size_t partials_bytes, void* stream) {
  const char* who = "gpz_spatial_stats";
  GPZ_REQUIRE(values && nbr && info && partials, "%s: null pointer", who);
  if (int rc = sc_check_args(who, N, L, K, dtype)) return rc;
  GPZ_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 15) == 0, "%s: partials must be 16-byte aligned", who);
  const ScPlan p = sc_plan(N, L, partials);
  GPZ_REQUIRE(partials_bytes >= p.bytes, "%s: partials too small (%zu bytes, %zu needed)", who, partials_bytes, p.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  GPZ_HIP_OK(hipMemsetAsync(info, 0, sizeof(int32_t), s));
  const SsOut o{I, C, mean, var, kurtosis};
  return dtype == GPZ_F32 ? sc_run<float>(values, N, L, nbr, K, o, info, p, s) : sc_run<double>(values, N, L, nbr, K, o, info, p, s);
}

extern "C" int gpz_gene_autocorr_perm_sparse_plan(int64_t N, int64_t D, int64_t nnz, int32_t K, int64_t P, int32_t stat,
                                                  int32_t perm_batch_wanted, int32_t line_mode_wanted, int32_t* perm_batch,
                                                  int32_t* line_mode, int32_t* workgroups, int64_t* partials_bytes) {
  const char* who = "gpz_gene_autocorr_perm_sparse";
  if (int rc = gr_check_shape(who, N, D, nnz)) return rc;
  if (int rc = ap_check_stat(who, stat)) return rc;
  return mp_plan_query(who, N, D, K, P, perm_batch_wanted, line_mode_wanted, true, perm_batch, line_mode, workgroups, partials_bytes);
}

extern "C" int gpz_gene_autocorr_perm_sparse(const int64_t* row_ptr, const int32_t* row_spot, const int32_t* row_perm,
                                             const float* col_val, const int64_t* nbr, const int32_t* perms, int64_t N, int64_t D,
                                             int64_t nnz, int32_t K, int64_t P, int32_t stat, int32_t perm_batch, int32_t line_mode,
                                             double* value, double* sims, int32_t* n_ge, int32_t* n_le, double* sim_mean,
                                             double* sim_m2, int32_t* info, void* partials, size_t partials_bytes, void* stream) {
  const char* who = "gpz_gene_autocorr_perm_sparse";
  GPZ_REQUIRE(row_ptr && nbr && perms && value && n_ge && n_le && sim_mean && sim_m2 && info && partials, "%s: null pointer", who);
  if (int rc = gr_check_shape(who, N, D, nnz)) return rc;
  if (int rc = ap_check_stat(who, stat)) return rc;
  GPZ_REQUIRE(nnz == 0 || (row_spot && row_perm && col_val), "%s: null pointer (non-zeros)", who);
  return mp_run_sparse(who, stat, GrRows{row_ptr, row_spot, row_perm, col_val, N, D, nnz}, nbr, perms, K, P, perm_batch, line_mode,
                       MpOut{value, sims, n_ge, n_le, sim_mean, sim_m2, info}, partials, partials_bytes, stream);
}

extern "C" int gpz_autocorr_perm_rows_plan(int64_t N, int64_t D, int32_t K, int64_t P, int32_t stat, int32_t perm_batch_wanted,
                                           int32_t line_mode_wanted, int32_t* perm_batch, int32_t* line_mode, int32_t* workgroups,
                                           int64_t* partials_bytes) {
  const char* who = "gpz_autocorr_perm_rows";
  if (int rc = gr_check_shape(who, N, D, 0)) return rc;
  if (int rc = ap_check_stat(who, stat)) return rc;
  return mp_plan_query(who, N, D, K, P, perm_batch_wanted, line_mode_wanted, false, perm_batch, line_mode, workgroups, partials_bytes);
}

extern "C" int gpz_autocorr_perm_rows(const float* values, const int64_t* nbr, const int32_t* perms, int64_t N, int64_t D, int32_t K,
                                      int64_t P, int32_t stat, int32_t perm_batch, int32_t line_mode, double* value, double* sims,
                                      int32_t* n_ge, int32_t* n_le, double* sim_mean, double* sim_m2, int32_t* info, void* partials,
                                      size_t partials_bytes, void* stream) {
  const char* who = "gpz_autocorr_perm_rows";
  GPZ_REQUIRE(values && nbr && perms && value && n_ge && n_le && sim_mean && sim_m2 && info && partials, "%s: null pointer", who);
  if (int rc = gr_check_shape(who, N, D, 0)) return rc;
  if (int rc = ap_check_stat(who, stat)) return rc;
  return mp_run_rows(who, stat, values, N, D, nbr, perms, K, P, perm_batch, line_mode,
                     MpOut{value, sims, n_ge, n_le, sim_mean, sim_m2, info}, partials, partials_bytes, stream);
}
