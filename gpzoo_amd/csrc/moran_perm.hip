// moran_perm.hip -- Moran's I or Geary's C of every gene under P relabellings of the spots: the permutation null of squidpy's
// spatial_autocorr(..., n_perms=) / PySAL's Moran and Geary, in O(entries x K) per permutation and never forming D x N.
// The kernels are templated on the statistic; all four entries, Moran-only or with the statistic as an argument, are here.
//
// For a permutation pi of the N spots the permuted gene is x^pi[i] = x[pi[i]].  Relabelling the graph instead of the values,
//   sum_i z[pi[i]] sum_{j in nbr(i)} z[pi[j]]  =  sum_a z[a] sum_m z[T_pi[a, m]],
//   T_pi[pi[i], m] = pi[nbr[i, m]],   indeg_pi[pi[i]] = indeg[i],
// so in the expansion of moran_expr.h S, Q and the entries of a gene stay and only C_pi = sum x lag_pi and
// A_pi = sum indeg_pi x change.  I_pi is moran_value of those sums; "I_pi >= I" is decided on moran_order, t = N C - S A, in
// fp64: exact for integer-valued data with |t| < 2^53, so ties count as ties on every run and every path.
//
// Per call: the in-degree pass and the gene pass of moran_expr.h give I, and S, Q, t per gene (the identity's sums, in the
// order gpz_gene_morans_i_sparse adds them).  Then per batch of permutations:
//   mp_relabel_kernel  writes T_pi (int32) and indeg_pi of the batch by the scatter above, counting the writes per target
//                      row with integer atomics: an entry of perms outside [0, N) or a row written twice raises info = 2
//                      (a row never written implies one of the two).  A bad entry of nbr or perms becomes -1 in T_pi.
//   mp_stat_kernel     one workgroup of MP_THREADS per gene at a time.  The gene's row is made available once -- scattered
//                      into a line of N floats (SparseRows), or it is its own line (DenseRows) -- and every wave then takes
//                      permutations of the batch: lane l adds the entries l + 64 u + 256 v (u < 4) of the row into its
//                      slot u, the slots and lanes are folded in the order of gr_gene_kernel's binary tree over 256
//                      partial sums, by register adds and a fixed shuffle tree.  No barrier per permutation, and with the
//                      identity for pi the sums are those of the gene pass, bit for bit.  The wave leaves I_pi and t_pi in
//                      LDS; after the batch one thread folds them into the gene's running n_ge, n_le, mean and M2
//                      (Welford) in permutation order, so nothing depends on perm_batch.
// The line is in the scratch memory (line_mode 1) or in dynamic LDS (2) where 4 N plus the batch arrays fit a workgroup's
// 160 KiB; the arithmetic is the same.  No floating-point atomics; every sum fp64 in a fixed order.
//
// STAT_GEARY: the gene pass is the wide instantiation of moran_expr.h's, the second sum per permutation is
// Q_in,pi = sum indeg_pi x^2 in the place of A_pi, the value is geary_value and "C_pi >= C" is decided on geary_order,
// Q_in - 2 C_s.  Everything else is shared.  The Moran-only entries (gpz_gene_morans_perm_sparse, gpz_morans_perm_rows) are the
// entries that take the statistic (gpz_gene_autocorr_perm_sparse, gpz_autocorr_perm_rows) with STAT_MORAN and their own name
// in the messages.
#include "moran_expr.h"
#include "moran_pass.h"

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

constexpr int MP_THREADS = 1024;              // 16 waves: permutations in flight per gene
constexpr int MP_WAVES = MP_THREADS / 64;
constexpr int MP_BATCH_MAX = 32;              // permutations per launch: the LDS arrays of I_pi and t_pi
constexpr int MP_BATCH_LDS = MP_WAVES;        // what the plan chooses: one permutation per wave with the line in LDS, half of
constexpr int MP_BATCH_GLOBAL = MP_WAVES / 2; // that with the line in the scratch memory -- the tables in flight share the L2
                                              // with the lines, and more of them at once cost time (measured: DESIGN.md section 5)
constexpr size_t MP_LDS_MAX = 160 * 1024;     // LDS of a CU; one workgroup may take all of it
constexpr size_t MP_LDS_HEAD = 2 * MP_BATCH_MAX * sizeof(double);
constexpr size_t MP_TABLE_BYTES = size_t(256) << 20;

__global__ __launch_bounds__(GR_THREADS) void mp_relabel_kernel(const int64_t* __restrict__ nbr, const int32_t* __restrict__ indeg,
                                                                const int32_t* __restrict__ perms, int64_t N, int K, int pb,
                                                                int32_t* __restrict__ T, int32_t* __restrict__ indeg_pi,
                                                                int32_t* __restrict__ written, int32_t* __restrict__ info) {
  const int64_t e = int64_t(blockIdx.x) * GR_THREADS + threadIdx.x;
  if (e >= int64_t(pb) * N) return;
  const int64_t p = e / N, i = e - p * N;
  const int32_t* __restrict__ pi = perms + p * N;
  const int64_t a = pi[i];
  if (a < 0 || a >= N || atomicAdd(written + p * N + a, 1) != 0) {
    *info = 2;
    return;
  }
  int32_t* __restrict__ row = T + (p * N + a) * K;
  for (int m = 0; m < K; ++m) {
    const int64_t j = nbr[i * K + m];
    int32_t v = -1;                                               // skipped by mp_stat_kernel
    if (j >= 0 && j < N && j != i) {
      const int32_t pj = pi[j];
      if (pj >= 0 && pj < N) v = pj;
    }
    row[m] = v;
  }
  if (indeg) indeg_pi[p * N + a] = indeg[i];                       // the column form (moran_pass.h) has no in-degrees
}

struct MpBatch {
  const int32_t* T;          // (pb, N, K)
  const int32_t* indeg_pi;   // (pb, N)
  const double* stats;       // (D, GR_STATS) of the gene pass
  float* lines;              // (workgroups, N), all zero between launches (line_mode 1, staged rows)
  double* sims;              // nullable (D, P)
  int32_t* n_ge;
  int32_t* n_le;
  double* mean;
  double* m2;
  int64_t P, p0;             // permutations of the call, first one of this batch
  int K, pb;
};

template <class Rows, bool LDS_LINE, int STAT>
__global__ __launch_bounds__(MP_THREADS) void mp_stat_kernel(Rows r, MpBatch b) {
  extern __shared__ __attribute__((aligned(16))) double mp_smem[];      // I_pi, t_pi of the batch, then the line
  double* const sI = mp_smem;
  double* const sT = mp_smem + MP_BATCH_MAX;
  const int64_t N = r.spots();
  const int K = b.K;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* line = nullptr;                                                // written by this workgroup
  if constexpr (LDS_LINE) line = reinterpret_cast<float*>(mp_smem + 2 * MP_BATCH_MAX);
  else if constexpr (Rows::STAGED) line = b.lines + int64_t(blockIdx.x) * N;
  if constexpr (LDS_LINE && Rows::STAGED) {
    for (int64_t n = threadIdx.x; n < N; n += MP_THREADS) line[n] = 0.0f;
    __syncthreads();
  }
  for (int64_t d = blockIdx.x; d < r.genes(); d += gridDim.x) {
    int64_t lo, hi;
    r.row(d, lo, hi);
    const float* src = line;
    if constexpr (Rows::STAGED) {
      for (int64_t k = lo + threadIdx.x; k < hi; k += MP_THREADS) {
        int32_t spot;
        float x;
        if (r.entry(lo, k, spot, x)) line[spot] = x;
      }
      __syncthreads();
    } else if constexpr (LDS_LINE) {
      const float* row = r.line(d);
      for (int64_t n = threadIdx.x; n < N; n += MP_THREADS) line[n] = row[n];
      __syncthreads();
    } else {
      src = r.line(d);
    }
    const double S = b.stats[d * GR_STATS + 0], Q = b.stats[d * GR_STATS + 1], t0 = b.stats[d * GR_STATS + 2];
    const bool scored = b.stats[d * GR_STATS + 3] != 0.0;
    for (int q = wave; q < b.pb; q += MP_WAVES) {
      const int32_t* __restrict__ T = b.T + int64_t(q) * N * K;
      const int32_t* __restrict__ dg = b.indeg_pi + int64_t(q) * N;
      double c[4] = {0.0, 0.0, 0.0, 0.0}, a[4] = {0.0, 0.0, 0.0, 0.0};
      for (int64_t base = lo; base < hi; base += GR_THREADS) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int64_t k = base + u * 64 + lane;
          int32_t spot;
          if (k >= hi || !r.spot_of(lo, k, spot)) continue;
          const double x = double(src[spot]);                           // the entry's value: what was scattered there
          const int32_t* __restrict__ row = T + int64_t(spot) * K;
          double lag = 0.0;
          for (int m = 0; m < K; ++m) {
            const int32_t j = row[m];
            if (j < 0 || j >= N) continue;                              // mp_relabel_kernel has told the caller
            lag += double(src[j]);
          }
          c[u] += x * lag;
          if constexpr (STAT == STAT_GEARY) a[u] += double(dg[spot]) * (x * x);
          else a[u] += double(dg[spot]) * x;
        }
      }
      // the tree of gr_gene_kernel over 256 partial sums: slots t and t + 128, then t and t + 64, then the lanes
      double cs = (c[0] + c[2]) + (c[1] + c[3]), as = (a[0] + a[2]) + (a[1] + a[3]);
      for (int h = 32; h >= 1; h >>= 1) {
        cs += __shfl_down(cs, h, 64);
        as += __shfl_down(as, h, 64);
      }
      if (lane == 0) {
        if constexpr (STAT == STAT_GEARY) {
          sI[q] = geary_value(N, K, S, Q, cs, as, scored);
          sT[q] = geary_order(cs, as);
        } else {
          sI[q] = moran_value(N, K, S, Q, cs, as, scored);
          sT[q] = moran_order(N, S, cs, as);
        }
      }
    }
    __syncthreads();                                                    // every gather of the line is done
    if constexpr (Rows::STAGED) {
      for (int64_t k = lo + threadIdx.x; k < hi; k += MP_THREADS) {
        int32_t spot;
        if (r.spot_of(lo, k, spot)) line[spot] = 0.0f;
      }
    }
    if (threadIdx.x == MP_THREADS - 1) {                                // the running summaries, in permutation order
      int32_t ge = b.n_ge[d], le = b.n_le[d];
      double mean = b.mean[d], m2 = b.m2[d];
      for (int q = 0; q < b.pb; ++q) {
        const double Iq = sI[q], tq = sT[q];
        const bool ok = Iq == Iq;                                       // a gene without I counts nothing
        ge += (ok && tq >= t0) ? 1 : 0;
        le += (ok && tq <= t0) ? 1 : 0;
        const double delta = Iq - mean;
        mean += delta / double(b.p0 + q + 1);
        m2 += delta * (Iq - mean);
        if (b.sims) b.sims[d * b.P + b.p0 + q] = Iq;
      }
      b.n_ge[d] = ge;
      b.n_le[d] = le;
      b.mean[d] = mean;
      b.m2[d] = m2;
    }
    __syncthreads();                                                    // the line is clear, the batch arrays are free
  }
}

struct MpPlan {
  double* stats;      // (D, GR_STATS)
  int32_t* T;         // (perm_batch, N, K)
  int32_t* indeg_pi;  // (perm_batch, N)
  int32_t* written;   // (perm_batch, N)
  int perm_batch, line_mode;
  size_t lds, bytes;
};

static int mp_check_stat(const char* who, int32_t stat) {
  GPZ_REQUIRE(stat == STAT_MORAN || stat == STAT_GEARY, "%s: stat %d unknown (0 Moran's I, 1 Geary's C)", who, stat);
  return 0;
}

// c has given the gene pass its share of the scratch memory (GenePass); the batch arrays follow it
static int mp_plan(const char* who, int64_t N, int64_t D, int32_t K, int64_t P, int32_t perm_batch, int32_t line_mode, Carver& c,
                   MpPlan& p) {
  if (int rc = gr_check_k(who, N, K)) return rc;
  GPZ_REQUIRE(P >= 1 && P < (1ll << 31), "%s: P = %lld permutations unsupported (1 <= P < 2^31)", who, (long long)P);
  GPZ_REQUIRE(perm_batch >= 0 && perm_batch <= MP_BATCH_MAX, "%s: perm_batch = %d unsupported (0 = chosen here, at most %d)", who,
              perm_batch, MP_BATCH_MAX);
  GPZ_REQUIRE(line_mode >= 0 && line_mode <= 2, "%s: line_mode %d unknown (0 chosen here, 1 scratch memory, 2 LDS)", who, line_mode);
  const bool fits = MP_LDS_HEAD + size_t(N) * sizeof(float) <= MP_LDS_MAX;
  GPZ_REQUIRE(line_mode != 2 || fits, "%s: a line of N = %lld floats does not fit a workgroup's LDS (%zu bytes with the batch arrays, %zu there)",
              who, (long long)N, MP_LDS_HEAD + size_t(N) * sizeof(float), MP_LDS_MAX);
  p = MpPlan{};
  p.line_mode = line_mode == 0 ? (fits ? 2 : 1) : line_mode;      // LDS wherever it fits (measured: DESIGN.md section 5)
  p.lds = MP_LDS_HEAD + (p.line_mode == 2 ? size_t(N) * sizeof(float) : 0);
  if (perm_batch == 0) {                                          // the tables of a batch take at most MP_TABLE_BYTES
    const size_t per = size_t(N) * size_t(K + 2) * sizeof(int32_t);
    const size_t fit = MP_TABLE_BYTES / per, cap = size_t(p.line_mode == 2 ? MP_BATCH_LDS : MP_BATCH_GLOBAL);
    perm_batch = int32_t(fit < 1 ? 1 : (fit > cap ? cap : fit));
  }
  p.perm_batch = int(perm_batch < P ? perm_batch : P);
  p.stats = c.take<double>(size_t(D) * GR_STATS);
  p.T = c.take<int32_t>(size_t(p.perm_batch) * size_t(N) * size_t(K));
  p.indeg_pi = c.take<int32_t>(size_t(p.perm_batch) * size_t(N));
  p.written = c.take<int32_t>(size_t(p.perm_batch) * size_t(N));
  p.bytes = c.used();
  return 0;
}

template <class Rows, bool LDS_LINE, int STAT>
static int mp_launch_stat(const Rows& r, const MpBatch& b, int workgroups, size_t lds, hipStream_t s) {
  if (LDS_LINE) {
    static bool set[64] = {};
    int dev = 0;
    GPZ_HIP_OK(hipGetDevice(&dev));
    if (!set[dev & 63]) {
      GPZ_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(&mp_stat_kernel<Rows, LDS_LINE, STAT>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, int(MP_LDS_MAX)));
      set[dev & 63] = true;
    }
  }
  hipLaunchKernelGGL((mp_stat_kernel<Rows, LDS_LINE, STAT>), dim3(unsigned(workgroups)), dim3(MP_THREADS), lds, s, r, b);
  GPZ_LAUNCH_OK();
  return 0;
}

template <class Rows, int STAT>
static int mp_run(const char* who, const Rows& r, const int64_t* nbr, const int32_t* perms, int64_t N, int64_t D, int32_t K, int64_t P,
                  int32_t perm_batch, int32_t line_mode, const MpOut& o, void* partials, size_t partials_bytes, void* stream) {
  GPZ_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 15) == 0, "%s: partials must be 16-byte aligned", who);
  Carver c(partials);
  const GenePass gene(c, N, D, Rows::STAGED);
  MpPlan p;
  if (int rc = mp_plan(who, N, D, K, P, perm_batch, line_mode, c, p)) return rc;
  GPZ_REQUIRE(partials_bytes >= p.bytes, "%s: partials too small (%zu bytes, %zu needed)", who, partials_bytes, p.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  GPZ_HIP_OK(hipMemsetAsync(o.n_ge, 0, size_t(D) * sizeof(int32_t), s));
  GPZ_HIP_OK(hipMemsetAsync(o.n_le, 0, size_t(D) * sizeof(int32_t), s));
  GPZ_HIP_OK(hipMemsetAsync(o.sim_mean, 0, size_t(D) * sizeof(double), s));
  GPZ_HIP_OK(hipMemsetAsync(o.sim_m2, 0, size_t(D) * sizeof(double), s));
  constexpr bool WIDE = STAT == STAT_GEARY;
  const SsOut observed{WIDE ? nullptr : o.I, WIDE ? o.I : nullptr, nullptr, nullptr, nullptr};
  if (int rc = gene.template run<WIDE>(r, nbr, N, int(K), observed, p.stats, o.info, s)) return rc;
  for (int64_t p0 = 0; p0 < P; p0 += p.perm_batch) {
    const int pb = int(P - p0 < p.perm_batch ? P - p0 : p.perm_batch);
    if (int rc = relabel_tables(nbr, gene.indeg, perms + p0 * N, N, int(K), pb, p.T, p.indeg_pi, p.written, o.info, s)) return rc;
    const MpBatch b{p.T, p.indeg_pi, p.stats, gene.lines, o.sims, o.n_ge, o.n_le, o.sim_mean, o.sim_m2, P, p0, int(K), pb};
    if (int rc = p.line_mode == 2 ? mp_launch_stat<Rows, true, STAT>(r, b, gene.workgroups, p.lds, s)
                                  : mp_launch_stat<Rows, false, STAT>(r, b, gene.workgroups, p.lds, s))
      return rc;
  }
  return 0;
}

// The four plan queries; staged = rows stored as their non-zeros (dense rows pass nnz = 0).
static int mp_query(const char* who, int64_t N, int64_t D, int64_t nnz, bool staged, int32_t K, int64_t P, int32_t stat,
                    int32_t perm_batch_wanted, int32_t line_mode_wanted, int32_t* perm_batch, int32_t* line_mode, int32_t* workgroups,
                    int64_t* partials_bytes) {
  if (int rc = gr_check_shape(who, N, D, nnz)) return rc;
  if (int rc = mp_check_stat(who, stat)) return rc;
  Carver c(nullptr);
  const GenePass gene(c, N, D, staged);
  MpPlan p;
  if (int rc = mp_plan(who, N, D, K, P, perm_batch_wanted, line_mode_wanted, c, p)) return rc;
  if (perm_batch) *perm_batch = p.perm_batch;
  if (line_mode) *line_mode = p.line_mode;
  if (workgroups) *workgroups = gene.workgroups;
  if (partials_bytes) *partials_bytes = int64_t(p.bytes);
  return 0;
}

// The four entries: the rows stored as their non-zeros (rows), or dense (values (D, N), and of rows the extents alone).
static int mp_entry(const char* who, int32_t stat, const GrRows& rows, const float* values, const int64_t* nbr, const int32_t* perms,
                    int32_t K, int64_t P, int32_t perm_batch, int32_t line_mode, const MpOut& o, void* partials, size_t partials_bytes,
                    void* stream) {
  const bool sparse = values == nullptr;
  GPZ_REQUIRE((!sparse || rows.row_ptr) && nbr && perms && o.I && o.n_ge && o.n_le && o.sim_mean && o.sim_m2 && o.info && partials,
              "%s: null pointer", who);
  if (int rc = gr_check_shape(who, rows.N, rows.D, rows.nnz)) return rc;
  if (int rc = mp_check_stat(who, stat)) return rc;
  GPZ_REQUIRE(!sparse || rows.nnz == 0 || (rows.row_spot && rows.row_perm && rows.col_val), "%s: null pointer (non-zeros)", who);
  auto run = [&](const auto& r) {
    using Rows = std::decay_t<decltype(r)>;
    return stat == STAT_GEARY ? mp_run<Rows, STAT_GEARY>(who, r, nbr, perms, rows.N, rows.D, K, P, perm_batch, line_mode, o, partials,
                                                         partials_bytes, stream)
                              : mp_run<Rows, STAT_MORAN>(who, r, nbr, perms, rows.N, rows.D, K, P, perm_batch, line_mode, o, partials,
                                                         partials_bytes, stream);
  };
  return sparse ? run(SparseRows{rows}) : run(DenseRows{values, rows.N, rows.D});
}

}  // namespace grk

// moran_pass.h: the tables of one batch, for the entries here and for the permutation column pass of spatial_stats.hip
int relabel_tables(const int64_t* nbr, const int32_t* indeg, const int32_t* perms, int64_t N, int K, int pb, int32_t* T,
                   int32_t* indeg_pi, int32_t* written, int32_t* info, hipStream_t s) {
  const int64_t rows = int64_t(pb) * N;
  GPZ_HIP_OK(hipMemsetAsync(written, 0, size_t(rows) * sizeof(int32_t), s));
  hipLaunchKernelGGL(grk::mp_relabel_kernel, dim3(unsigned((rows + grk::GR_THREADS - 1) / grk::GR_THREADS)), dim3(grk::GR_THREADS), 0,
                     s, nbr, indeg, perms, N, K, pb, T, indeg_pi, written, info);
  GPZ_LAUNCH_OK();
  return 0;
}

}  // namespace gpz

using namespace gpz;
using namespace gpz::grk;

extern "C" int gpz_gene_autocorr_perm_sparse_plan(int64_t N, int64_t D, int64_t nnz, int32_t K, int64_t P, int32_t stat,
                                                  int32_t perm_batch_wanted, int32_t line_mode_wanted, int32_t* perm_batch,
                                                  int32_t* line_mode, int32_t* workgroups, int64_t* partials_bytes) {
  return mp_query("gpz_gene_autocorr_perm_sparse", N, D, nnz, true, K, P, stat, perm_batch_wanted, line_mode_wanted, perm_batch,
                  line_mode, workgroups, partials_bytes);
}

extern "C" int gpz_gene_morans_perm_sparse_plan(int64_t N, int64_t D, int64_t nnz, int32_t K, int64_t P, int32_t perm_batch_wanted,
                                                int32_t line_mode_wanted, int32_t* perm_batch, int32_t* line_mode,
                                                int32_t* workgroups, int64_t* partials_bytes) {
  return mp_query("gpz_gene_morans_perm_sparse", N, D, nnz, true, K, P, STAT_MORAN, perm_batch_wanted, line_mode_wanted, perm_batch,
                  line_mode, workgroups, partials_bytes);
}

extern "C" int gpz_autocorr_perm_rows_plan(int64_t N, int64_t D, int32_t K, int64_t P, int32_t stat, int32_t perm_batch_wanted,
                                           int32_t line_mode_wanted, int32_t* perm_batch, int32_t* line_mode, int32_t* workgroups,
                                           int64_t* partials_bytes) {
  return mp_query("gpz_autocorr_perm_rows", N, D, 0, false, K, P, stat, perm_batch_wanted, line_mode_wanted, perm_batch, line_mode,
                  workgroups, partials_bytes);
}

extern "C" int gpz_morans_perm_rows_plan(int64_t N, int64_t D, int32_t K, int64_t P, int32_t perm_batch_wanted,
                                         int32_t line_mode_wanted, int32_t* perm_batch, int32_t* line_mode, int32_t* workgroups,
                                         int64_t* partials_bytes) {
  return mp_query("gpz_morans_perm_rows", N, D, 0, false, K, P, STAT_MORAN, perm_batch_wanted, line_mode_wanted, perm_batch, line_mode,
                  workgroups, partials_bytes);
}

extern "C" int gpz_gene_autocorr_perm_sparse(const int64_t* row_ptr, const int32_t* row_spot, const int32_t* row_perm,
                                             const float* col_val, const int64_t* nbr, const int32_t* perms, int64_t N, int64_t D,
                                             int64_t nnz, int32_t K, int64_t P, int32_t stat, int32_t perm_batch, int32_t line_mode,
                                             double* value, double* sims, int32_t* n_ge, int32_t* n_le, double* sim_mean,
                                             double* sim_m2, int32_t* info, void* partials, size_t partials_bytes, void* stream) {
  return mp_entry("gpz_gene_autocorr_perm_sparse", stat, GrRows{row_ptr, row_spot, row_perm, col_val, N, D, nnz}, nullptr, nbr, perms, K,
                  P, perm_batch, line_mode, MpOut{value, sims, n_ge, n_le, sim_mean, sim_m2, info}, partials, partials_bytes, stream);
}

extern "C" int gpz_gene_morans_perm_sparse(const int64_t* row_ptr, const int32_t* row_spot, const int32_t* row_perm,
                                           const float* col_val, const int64_t* nbr, const int32_t* perms, int64_t N, int64_t D,
                                           int64_t nnz, int32_t K, int64_t P, int32_t perm_batch, int32_t line_mode, double* I,
                                           double* sims, int32_t* n_ge, int32_t* n_le, double* sim_mean, double* sim_m2,
                                           int32_t* info, void* partials, size_t partials_bytes, void* stream) {
  return mp_entry("gpz_gene_morans_perm_sparse", STAT_MORAN, GrRows{row_ptr, row_spot, row_perm, col_val, N, D, nnz}, nullptr, nbr,
                  perms, K, P, perm_batch, line_mode, MpOut{I, sims, n_ge, n_le, sim_mean, sim_m2, info}, partials, partials_bytes,
                  stream);
}

extern "C" int gpz_autocorr_perm_rows(const float* values, const int64_t* nbr, const int32_t* perms, int64_t N, int64_t D, int32_t K,
                                      int64_t P, int32_t stat, int32_t perm_batch, int32_t line_mode, double* value, double* sims,
                                      int32_t* n_ge, int32_t* n_le, double* sim_mean, double* sim_m2, int32_t* info, void* partials,
                                      size_t partials_bytes, void* stream) {
  GPZ_REQUIRE(values, "gpz_autocorr_perm_rows: null pointer");
  return mp_entry("gpz_autocorr_perm_rows", stat, GrRows{nullptr, nullptr, nullptr, nullptr, N, D, 0}, values, nbr, perms, K, P,
                  perm_batch, line_mode, MpOut{value, sims, n_ge, n_le, sim_mean, sim_m2, info}, partials, partials_bytes, stream);
}

extern "C" int gpz_morans_perm_rows(const float* values, const int64_t* nbr, const int32_t* perms, int64_t N, int64_t D, int32_t K,
                                    int64_t P, int32_t perm_batch, int32_t line_mode, double* I, double* sims, int32_t* n_ge,
                                    int32_t* n_le, double* sim_mean, double* sim_m2, int32_t* info, void* partials,
                                    size_t partials_bytes, void* stream) {
  GPZ_REQUIRE(values, "gpz_morans_perm_rows: null pointer");
  return mp_entry("gpz_morans_perm_rows", STAT_MORAN, GrRows{nullptr, nullptr, nullptr, nullptr, N, D, 0}, values, nbr, perms, K, P,
                  perm_batch, line_mode, MpOut{I, sims, n_ge, n_le, sim_mean, sim_m2, info}, partials, partials_bytes, stream);
}

