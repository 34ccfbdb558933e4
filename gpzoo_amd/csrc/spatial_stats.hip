// spatial_stats.hip -- Moran's I of the columns of a dense array, and Geary's C, the mean, the variance and the kurtosis beside
// it: squidpy's spatial_autocorr(mode="moran" | "geary") / PySAL's Moran and Geary with what their randomisation moments
// (VI_rand, VC_rand) need of each column or gene, b2 = m4 / m2^2.
//
// The column pass, one pair of kernels instantiated narrow (I, and the variance where asked for) and wide (all five):
//   mi_rows<TERMS = false>   per chunk of 256 rows: column sums of v - v[0] (shifted by the column's first value, so a
//                            constant column has a mean equal to its value and gives 0 / 0 = NaN)
//   mi_rows<TERMS = true>    per chunk: sum_i z_i * (mean of z over i's neighbours) and sum_i z_i^2, z = v - mean; wide also
//                            G = sum_i sum_j (z_i - z_j)^2, a sum of non-negative terms, and sum z^4
//   mi_final                 per column: the chunks' partials in a fixed order -> the mean, then I = numerator / denominator
//                            and the rest
// The narrow instantiation adds what the wide one adds to its first two sums, so I has the same bits from either.
//   gpz_morans_i             narrow, the first L columns of an (N, L) array, fp32 or fp64
//   moran_slab_run           narrow, the columns of an fp32 residual slab wider than what is scored (moran_pass.h; residual.hip)
//   moran_slab_wide_run      wide, the same columns; moran_slab_perm_run scores them under relabelled tables (further down)
//   gpz_spatial_stats        wide, as gpz_morans_i takes its columns
//   gpz_gene_spatial_stats_sparse   the by-gene arrays of a whole data set stored as its non-zeros: the wide instantiation of
//                            the gene pass of moran_expr.h.  I has gpz_gene_morans_i_sparse's bits.
// Built with -ffp-contract=off: every product and sum is rounded on its own, as in gene_rank.hip and moran_perm.hip, whose
// bits the gene entry has to give.  No floating-point atomics; every sum fp64 in a fixed order: two calls agree bit for bit.
#include "moran_expr.h"
#include "moran_pass.h"

namespace gpz {
namespace grk {

constexpr int MI_THREADS = 256;
constexpr int MI_ROWS = 256;         // rows per partial sum

// per (chunk, column): shifted sum, sum z lag / K, sum z^2, and wide: G, sum z^4
constexpr int mi_part(bool wide) { return wide ? 5 : 3; }

// Threads of a block: cw columns x (MI_THREADS / cw) row slots; cw = the power of two >= L, at most 64.
static int mi_cw(int64_t L) {
  int cw = 1;
  while (cw < L && cw < 64) cw <<= 1;
  return cw;
}

struct MiPlan {
  double* part;       // (chunks, L, mi_part(wide))
  double* mean;       // (L,)
  int64_t chunks;
  size_t bytes;
};

static MiPlan mi_plan(int64_t N, int64_t L, bool wide, void* scratch) {
  Carver c(scratch);
  MiPlan p{};
  p.chunks = (N + MI_ROWS - 1) / MI_ROWS;
  p.part = c.take<double>(size_t(p.chunks) * size_t(L) * mi_part(wide));
  p.mean = c.take<double>(size_t(L));
  p.bytes = c.used();
  return p;
}

// Block (chunk, column tile): each thread sums its rows in order, then row slot 0 adds the slots in order.  V holds N rows
// of ld values each, of which the first L are the columns (ld = L for the entries; a residual slab is wider).
template <typename T, bool TERMS, bool WIDE>
__global__ __launch_bounds__(MI_THREADS) void mi_rows(const T* __restrict__ V, int64_t N, int64_t L, int64_t ld, int cw,
                                                      const int64_t* __restrict__ nbr, int K, const double* __restrict__ mean,
                                                      double* __restrict__ part, int32_t* __restrict__ info) {
  constexpr int SUMS = WIDE ? 4 : 2;
  __shared__ double red[SUMS][MI_THREADS];
  const int c = threadIdx.x % cw, slot = threadIdx.x / cw, slots = MI_THREADS / cw;
  const int64_t l = int64_t(blockIdx.y) * cw + c;
  const int64_t r0 = int64_t(blockIdx.x) * MI_ROWS, r1 = r0 + MI_ROWS < N ? r0 + MI_ROWS : N;
  double a = 0.0, b = 0.0, g = 0.0, f = 0.0;
  if (l < L) {
    const double ref = TERMS ? mean[l] : double(V[l]);
    const double w = 1.0 / K;
    for (int64_t i = r0 + slot; i < r1; i += slots) {
      const double z = double(V[i * ld + l]) - ref;
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
        const double zj = double(V[j * ld + l]) - ref;
        lag += zj;
        if constexpr (WIDE) gi += (z - zj) * (z - zj);
      }
      const double z2 = z * z;
      a += z * (lag * w);
      b += z2;
      if constexpr (WIDE) {
        g += gi;
        f += z2 * z2;
      }
    }
  }
  red[0][threadIdx.x] = a;
  red[1][threadIdx.x] = b;
  if constexpr (WIDE) {
    red[2][threadIdx.x] = g;
    red[3][threadIdx.x] = f;
  }
  __syncthreads();
  if (slot == 0 && l < L) {
    for (int r = 1; r < slots; ++r) {
      a += red[0][r * cw + c];
      b += red[1][r * cw + c];
      if constexpr (WIDE) {
        g += red[2][r * cw + c];
        f += red[3][r * cw + c];
      }
    }
    double* o = part + (int64_t(blockIdx.x) * L + l) * mi_part(WIDE);
    if (TERMS) {
      o[1] = a;
      o[2] = b;
      if constexpr (WIDE) {
        o[3] = g;
        o[4] = f;
      }
    } else {
      o[0] = a;
    }
  }
}

// Block = column: the chunks' partials in a fixed order (strided per thread, then a fixed tree).  TERMS == false: the mean
// (first value + shifted sum / N) into `mean` and, wide, where asked for, o.mean.  TERMS == true: I = numerator / denominator
// (0 / 0 = NaN: a constant column) and the variance, denominator / N, where asked for; wide, every field of o that is not null.
template <typename T, bool TERMS, bool WIDE>
__global__ __launch_bounds__(MI_THREADS) void mi_final(const double* __restrict__ part, int64_t chunks, int64_t L, int64_t N, int K,
                                                       const T* __restrict__ V, double* __restrict__ mean, SsOut o) {
  constexpr int SUMS = WIDE ? 4 : 2;
  __shared__ double red[SUMS][MI_THREADS];
  const int64_t l = blockIdx.x;
  double a = 0.0, b = 0.0, g = 0.0, f = 0.0;
  for (int64_t ch = threadIdx.x; ch < chunks; ch += MI_THREADS) {
    const double* p = part + (ch * L + l) * mi_part(WIDE);
    if (TERMS) {
      a += p[1];
      b += p[2];
      if constexpr (WIDE) {
        g += p[3];
        f += p[4];
      }
    } else {
      a += p[0];
    }
  }
  red[0][threadIdx.x] = a;
  red[1][threadIdx.x] = b;
  if constexpr (WIDE) {
    red[2][threadIdx.x] = g;
    red[3][threadIdx.x] = f;
  }
  __syncthreads();
  for (int h = MI_THREADS / 2; h >= 1; h >>= 1) {
    if (int(threadIdx.x) < h)
      for (int v = 0; v < SUMS; ++v) red[v][threadIdx.x] += red[v][threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  if (!TERMS) {
    const double m = double(V[l]) + red[0][0] / double(N);
    mean[l] = m;
    if (WIDE && o.mean) o.mean[l] = m;
    return;
  }
  const double Nd = double(N), den = red[1][0], var = den / Nd;          // 0 / 0 = NaN: a constant column
  if (!WIDE || o.I) o.I[l] = red[0][0] / den;
  if (o.var) o.var[l] = var;
  if constexpr (WIDE) {
    if (o.C) o.C[l] = ((Nd - 1.0) * red[2][0]) / (2.0 * Nd * double(K) * den);
    if (o.kurtosis) o.kurtosis[l] = (red[3][0] / Nd) / (var * var);
  }
}

// The four launches over the first L columns of V (N rows of ld values); the means are left in pl.mean.
template <typename T, bool WIDE>
static int mi_run(const void* values, int64_t N, int64_t L, int64_t ld, const int64_t* nbr, int K, const SsOut& o, int32_t* info,
                  const MiPlan& pl, hipStream_t s) {
  const T* V = static_cast<const T*>(values);
  const int cw = mi_cw(L);
  const dim3 rows(unsigned(pl.chunks), unsigned((L + cw - 1) / cw)), block(MI_THREADS);
  hipLaunchKernelGGL((mi_rows<T, false, WIDE>), rows, block, 0, s, V, N, L, ld, cw, nbr, K, pl.mean, pl.part, info);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL((mi_final<T, false, WIDE>), dim3(unsigned(L)), block, 0, s, pl.part, pl.chunks, L, N, K, V, pl.mean, o);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL((mi_rows<T, true, WIDE>), rows, block, 0, s, V, N, L, ld, cw, nbr, K, pl.mean, pl.part, info);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL((mi_final<T, true, WIDE>), dim3(unsigned(L)), block, 0, s, pl.part, pl.chunks, L, N, K, V, pl.mean, o);
  GPZ_LAUNCH_OK();
  return 0;
}

static int mi_check_args(const char* who, int64_t N, int64_t L, int32_t K, int32_t dtype) {
  GPZ_REQUIRE(dtype == GPZ_F32 || dtype == GPZ_F64, "%s: unknown dtype %d", who, dtype);
  GPZ_REQUIRE(K >= 1 && N > K && N < (int64_t(1) << 31), "%s: N=%lld, K=%d unsupported (1 <= K < N < 2^31)", who, (long long)N, K);
  GPZ_REQUIRE(L >= 1 && L <= (int64_t(1) << 20), "%s: L=%lld unsupported (1..2^20)", who, (long long)L);
  return 0;
}

// ---- the permutation column pass (moran_pass.h) ------------------------------------------------------------------------
// For a column z, centred by the mean the wide pass left, sum z^2, sum z^4 and the mean do not change under a relabelling
// of the rows; a_pi = sum_a z_a (1 / K) sum_m z[T_pi[a, m]] and G_pi = sum_a sum_m (z_a - z[T_pi[a, m]])^2 do.
//   rp_rows<STAT, FULL>   block (chunk of 256 rows, column tile), the threads of mi_rows (cw columns x row slots), for a
//                         batch of up to RP_BATCH permutations: a thread reads its row's value once per batch and gathers,
//                         per permutation, the K neighbours named by the relabelled table -- each a row of the slab,
//                         contiguous over the tile's columns (whole 256-byte segments at cw = 64), RP_KU of them requested
//                         together.  One accumulator per permutation in registers; the row slots are folded as mi_rows
//                         folds them, RP_GROUP permutations per pair of barriers.  FULL (cw = 64): a wave is one row slot,
//                         so the table row's address is wave-uniform and can be read by scalar loads.
//   rp_observed           per column: the observed numerators and the denominator from the wide pass's partials, in
//                         mi_final's order (they are the sums I and C were divided from)
//   rp_final<STAT>        block = column, wave = permutation: the chunks' partials in mi_final's order (strided over 256
//                         virtual threads -- four registers of 64 lanes -- then its tree: registers, then shuffles), the
//                         value by mi_final's expression; then one thread folds the batch into the column's running
//                         n_ge, n_le, mean and M2 (Welford) in permutation order, so nothing depends on the batch size.
// With the identity for pi every sum is the wide pass's, bit for bit.
constexpr int RP_BATCH = SLAB_PERM_BATCH_MAX;
constexpr int RP_GROUP = 8;
constexpr int RP_KU = 8;
constexpr int RP_MORAN = 0, RP_GEARY = 1;

template <int STAT, bool FULL>
__global__ __launch_bounds__(MI_THREADS) void rp_rows(const float* __restrict__ V, int64_t N, int64_t L, int64_t ld, int cw,
                                                      const int32_t* __restrict__ T, int K, int pb, const double* __restrict__ mean,
                                                      double* __restrict__ part) {
  __shared__ double red[RP_GROUP][MI_THREADS];
  const int c = FULL ? int(threadIdx.x & 63) : int(threadIdx.x) % cw;
  const int slot = FULL ? __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)) : int(threadIdx.x) / cw;
  const int slots = MI_THREADS / cw;
  const int64_t l = int64_t(blockIdx.y) * cw + c;
  const int64_t r0 = int64_t(blockIdx.x) * MI_ROWS, r1 = r0 + MI_ROWS < N ? r0 + MI_ROWS : N;
  double acc[RP_BATCH];
#pragma unroll
  for (int q = 0; q < RP_BATCH; ++q) acc[q] = 0.0;
  if (l < L) {
    const double ref = mean[l];
    const double w = 1.0 / K;
    for (int64_t i = r0 + slot; i < r1; i += slots) {
      const double z = double(V[i * ld + l]) - ref;
#pragma unroll
      for (int q = 0; q < RP_BATCH; ++q) {
        if (q < pb) {
          const int32_t* __restrict__ row = T + (int64_t(q) * N + i) * K;
          double lag = 0.0, gi = 0.0;
          for (int k0 = 0; k0 < K; k0 += RP_KU) {
            int32_t j[RP_KU];
            float v[RP_KU];
#pragma unroll
            for (int u = 0; u < RP_KU; ++u) j[u] = k0 + u < K ? row[k0 + u] : -1;
#pragma unroll
            for (int u = 0; u < RP_KU; ++u) {
              j[u] = (j[u] >= 0 && j[u] < N) ? j[u] : -1;         // never read outside the slab; the relabel kernel has told the caller
              v[u] = V[(j[u] >= 0 ? int64_t(j[u]) : i) * ld + l];  // no branch between the requests: a skipped entry reads row i
            }
#pragma unroll
            for (int u = 0; u < RP_KU; ++u) {
              if (j[u] < 0) continue;
              const double zj = double(v[u]) - ref;
              if constexpr (STAT == RP_GEARY) gi += (z - zj) * (z - zj);
              else lag += zj;
            }
          }
          if constexpr (STAT == RP_GEARY) acc[q] += gi;
          else acc[q] += z * (lag * w);
        }
      }
    }
  }
#pragma unroll
  for (int g0 = 0; g0 < RP_BATCH; g0 += RP_GROUP) {
    if (g0 < pb) {                                                // the same for every thread of the block
#pragma unroll
      for (int u = 0; u < RP_GROUP; ++u) red[u][threadIdx.x] = acc[g0 + u];
      __syncthreads();
      if (slot == 0 && l < L) {
#pragma unroll
        for (int u = 0; u < RP_GROUP; ++u) {
          if (g0 + u >= pb) continue;
          double a = acc[g0 + u];
          for (int r = 1; r < slots; ++r) a += red[u][r * cw + c];
          part[(int64_t(g0 + u) * gridDim.x + blockIdx.x) * L + l] = a;
        }
      }
      __syncthreads();
    }
  }
}

// the sum of p[ch * stride], ch < chunks, as mi_final adds it: thread t of 256 takes ch = t, t + 256, ..., then the tree over
// the 256 sums.  Lane l holds threads l, l + 64, l + 128, l + 192; the result is lane 0's.
__device__ __forceinline__ double rp_fold(const double* __restrict__ p, int64_t stride, int64_t chunks, int lane) {
  double v[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int u = 0; u < 4; ++u)
    for (int64_t ch = lane + 64 * u; ch < chunks; ch += MI_THREADS) v[u] += p[ch * stride];
  double t = (v[0] + v[2]) + (v[1] + v[3]);
  for (int h = 32; h >= 1; h >>= 1) t += __shfl_down(t, h, 64);
  return t;
}

// obs (L, 3): sum z lag / K, sum z^2, G of the unpermuted column, from the wide pass's partials (chunks, L, 5)
__global__ __launch_bounds__(MI_THREADS) void rp_observed(const double* __restrict__ wide, int64_t chunks, int64_t L,
                                                          double* __restrict__ obs) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  const int64_t l = blockIdx.x;
  if (wave >= 3) return;
  const double t = rp_fold(wide + l * mi_part(true) + 1 + wave, L * mi_part(true), chunks, lane);
  if (lane == 0) obs[l * 3 + wave] = t;
}

template <int STAT>
__global__ __launch_bounds__(MI_THREADS) void rp_final(const double* __restrict__ part, int64_t chunks, int64_t L, int64_t N, int K,
                                                       int pb, int64_t p0, int64_t P, const double* __restrict__ obs, SlabPermOut o) {
  __shared__ double sV[RP_BATCH], sT[RP_BATCH];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  const int64_t l = blockIdx.x;
  const double Nd = double(N), den = obs[l * 3 + 1];
  for (int q = wave; q < pb; q += MI_THREADS / 64) {
    const double t = rp_fold(part + int64_t(q) * chunks * L + l, L, chunks, lane);
    if (lane == 0) {
      sT[q] = t;
      sV[q] = STAT == RP_GEARY ? ((Nd - 1.0) * t) / (2.0 * Nd * double(K) * den) : t / den;      // mi_final's expressions
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double t0 = obs[l * 3 + (STAT == RP_GEARY ? 2 : 0)];
  int32_t ge = o.n_ge[l], le = o.n_le[l];
  double mean = o.sim_mean[l], m2 = o.sim_m2[l];
  for (int q = 0; q < pb; ++q) {
    const double vq = sV[q], tq = sT[q];
    const bool ok = vq == vq;                                     // a constant column counts nothing
    ge += (ok && tq >= t0) ? 1 : 0;
    le += (ok && tq <= t0) ? 1 : 0;
    const double delta = vq - mean;
    mean += delta / double(p0 + q + 1);
    m2 += delta * (vq - mean);
    if (o.sims) o.sims[l * o.sims_ld + p0 + q] = vq;
  }
  o.n_ge[l] = ge;
  o.n_le[l] = le;
  o.sim_mean[l] = mean;
  o.sim_m2[l] = m2;
}

struct RpPlan {
  int32_t* T;         // (perm_batch, B, K)
  int32_t* written;   // (perm_batch, B)
  double* part;       // (perm_batch, chunks, cols)
  double* obs;        // (cols, 3)
  int64_t chunks;
  size_t bytes;
};

static RpPlan rp_plan(int64_t B, int64_t cols, int K, int pb, void* scratch) {
  Carver c(scratch);
  RpPlan p{};
  p.chunks = (B + MI_ROWS - 1) / MI_ROWS;
  p.T = c.take<int32_t>(size_t(pb) * size_t(B) * size_t(K));
  p.written = c.take<int32_t>(size_t(pb) * size_t(B));
  p.part = c.take<double>(size_t(pb) * size_t(p.chunks) * size_t(cols));
  p.obs = c.take<double>(size_t(cols) * 3);
  p.bytes = c.used();
  return p;
}

template <int STAT>
static int rp_run(const float* slab, int64_t B, int64_t cols, int64_t ld, const int64_t* nbr, int K, const int32_t* perms, int64_t P,
                  int perm_batch, const double* mean, const SlabPermOut& o, const RpPlan& pl, hipStream_t s) {
  const int cw = mi_cw(cols);
  const dim3 rows(unsigned(pl.chunks), unsigned((cols + cw - 1) / cw)), block(MI_THREADS);
  for (int64_t p0 = 0; p0 < P; p0 += perm_batch) {
    const int pb = int(P - p0 < perm_batch ? P - p0 : perm_batch);
    if (int rc = relabel_tables(nbr, nullptr, perms + p0 * B, B, K, pb, pl.T, nullptr, pl.written, o.info, s)) return rc;
    if (cw == 64) hipLaunchKernelGGL((rp_rows<STAT, true>), rows, block, 0, s, slab, B, cols, ld, cw, pl.T, K, pb, mean, pl.part);
    else hipLaunchKernelGGL((rp_rows<STAT, false>), rows, block, 0, s, slab, B, cols, ld, cw, pl.T, K, pb, mean, pl.part);
    GPZ_LAUNCH_OK();
    hipLaunchKernelGGL((rp_final<STAT>), dim3(unsigned(cols)), block, 0, s, pl.part, pl.chunks, cols, B, K, pb, p0, P, pl.obs, o);
    GPZ_LAUNCH_OK();
  }
  return 0;
}

}  // namespace grk

// moran_pass.h: the same four launches over a residual slab, with the column means and variances as outputs
size_t moran_slab_bytes(int64_t B, int64_t cols) { return grk::mi_plan(B, cols, false, nullptr).bytes; }

int moran_slab_run(const float* slab, int64_t B, int64_t cols, int64_t ld, const int64_t* nbr, int K, double* I, double* mean,
                   double* var, int32_t* info, void* scratch, hipStream_t s) {
  grk::MiPlan pl = grk::mi_plan(B, cols, false, scratch);
  pl.mean = mean;
  return grk::mi_run<float, false>(slab, B, cols, ld, nbr, K, grk::SsOut{I, nullptr, nullptr, var, nullptr}, info, pl, s);
}

// the wide instantiation over the same columns; its partials stay where moran_slab_perm_run looks for them
size_t moran_slab_wide_bytes(int64_t B, int64_t cols) { return grk::mi_plan(B, cols, true, nullptr).bytes; }

int moran_slab_wide_run(const float* slab, int64_t B, int64_t cols, int64_t ld, const int64_t* nbr, int K, double* I, double* C,
                        double* mean, double* var, double* kurtosis, int32_t* info, void* scratch, hipStream_t s) {
  grk::MiPlan pl = grk::mi_plan(B, cols, true, scratch);
  pl.mean = mean;
  return grk::mi_run<float, true>(slab, B, cols, ld, nbr, K, grk::SsOut{I, C, nullptr, var, kurtosis}, info, pl, s);
}

size_t moran_slab_perm_bytes(int64_t B, int64_t cols, int K, int perm_batch) {
  return grk::rp_plan(B, cols, K, perm_batch, nullptr).bytes;
}

int moran_slab_perm_run(const float* slab, int64_t B, int64_t cols, int64_t ld, const int64_t* nbr, int K, int stat,
                        const int32_t* perms, int64_t P, int perm_batch, const double* mean, const void* wide_scratch,
                        const SlabPermOut& o, void* scratch, hipStream_t s) {
  const grk::RpPlan pl = grk::rp_plan(B, cols, K, perm_batch, scratch);
  const grk::MiPlan wide = grk::mi_plan(B, cols, true, const_cast<void*>(wide_scratch));
  hipLaunchKernelGGL(grk::rp_observed, dim3(unsigned(cols)), dim3(grk::MI_THREADS), 0, s, wide.part, wide.chunks, cols, pl.obs);
  GPZ_LAUNCH_OK();
  return stat == grk::RP_GEARY ? grk::rp_run<grk::RP_GEARY>(slab, B, cols, ld, nbr, K, perms, P, perm_batch, mean, o, pl, s)
                               : grk::rp_run<grk::RP_MORAN>(slab, B, cols, ld, nbr, K, perms, P, perm_batch, mean, o, pl, s);
}

}  // namespace gpz

using namespace gpz;
using namespace gpz::grk;

extern "C" size_t gpz_morans_i_workspace_bytes(int64_t N, int64_t L, int32_t K) {
  if (mi_check_args("gpz_morans_i", N, L, K, GPZ_F64)) return 0;
  return mi_plan(N, L, false, nullptr).bytes;
}

extern "C" int gpz_morans_i(const void* values, int64_t N, int64_t L, int32_t dtype, const int64_t* nbr, int32_t K,
                            double* I, int32_t* info, void* ws, size_t ws_bytes, void* stream) {
  GPZ_REQUIRE(values && nbr && I && info && ws, "gpz_morans_i: null pointer");
  if (int rc = mi_check_args("gpz_morans_i", N, L, K, dtype)) return rc;
  const MiPlan pl = mi_plan(N, L, false, ws);
  GPZ_REQUIRE(ws_bytes >= pl.bytes, "gpz_morans_i: workspace of %zu bytes, %zu needed", ws_bytes, pl.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  GPZ_HIP_OK(hipMemsetAsync(info, 0, sizeof(int32_t), s));
  const SsOut o{I, nullptr, nullptr, nullptr, nullptr};
  return dtype == GPZ_F32 ? mi_run<float, false>(values, N, L, L, nbr, K, o, info, pl, s)
                          : mi_run<double, false>(values, N, L, L, nbr, K, o, info, pl, s);
}

extern "C" int gpz_spatial_stats_plan(int64_t N, int64_t L, int32_t K, int32_t* row_chunk, int64_t* chunks, int64_t* partials_bytes) {
  if (int rc = mi_check_args("gpz_spatial_stats", N, L, K, GPZ_F64)) return rc;
  const MiPlan p = mi_plan(N, L, true, nullptr);
  if (row_chunk) *row_chunk = MI_ROWS;
  if (chunks) *chunks = p.chunks;
  if (partials_bytes) *partials_bytes = int64_t(p.bytes);
  return 0;
}

extern "C" int gpz_spatial_stats(const void* values, int64_t N, int64_t L, int32_t dtype, const int64_t* nbr, int32_t K, double* I,
                                 double* C, double* mean, double* var, double* kurtosis, int32_t* info, void* partials,
                                 size_t partials_bytes, void* stream) {
  const char* who = "gpz_spatial_stats";
  GPZ_REQUIRE(values && nbr && info && partials, "%s: null pointer", who);
  if (int rc = mi_check_args(who, N, L, K, dtype)) return rc;
  GPZ_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 15) == 0, "%s: partials must be 16-byte aligned", who);
  const MiPlan p = mi_plan(N, L, true, partials);
  GPZ_REQUIRE(partials_bytes >= p.bytes, "%s: partials too small (%zu bytes, %zu needed)", who, partials_bytes, p.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  GPZ_HIP_OK(hipMemsetAsync(info, 0, sizeof(int32_t), s));
  const SsOut o{I, C, mean, var, kurtosis};
  return dtype == GPZ_F32 ? mi_run<float, true>(values, N, L, L, nbr, K, o, info, p, s)
                          : mi_run<double, true>(values, N, L, L, nbr, K, o, info, p, s);
}

extern "C" int gpz_gene_spatial_stats_sparse_plan(int64_t N, int64_t D, int64_t nnz, int32_t K, int32_t* gene_chunk,
                                                  int32_t* workgroups, int64_t* partials_bytes) {
  return gene_pass_query("gpz_gene_spatial_stats_sparse", N, D, nnz, K, gene_chunk, workgroups, partials_bytes);
}

extern "C" int gpz_gene_spatial_stats_sparse(const int64_t* row_ptr, const int32_t* row_spot, const int32_t* row_perm,
                                             const float* col_val, const int64_t* nbr, int64_t N, int64_t D, int64_t nnz, int32_t K,
                                             double* I, double* C, double* mean, double* var, double* kurtosis, int32_t* info,
                                             void* partials, size_t partials_bytes, void* stream) {
  return gene_pass_entry<true>("gpz_gene_spatial_stats_sparse", GrRows{row_ptr, row_spot, row_perm, col_val, N, D, nnz}, nbr, K,
                               SsOut{I, C, mean, var, kurtosis}, info, partials, partials_bytes, stream);
}
