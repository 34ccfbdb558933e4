// gene_gp.hip -- the two device steps of utilities.gene_spatial_gp, the sparse-GP test for spatially variable genes (what
// SpatialDE and nnSVG answer per gene: is it spatially variable under a GP, at what length scale, with what fraction of its
// variance), scored by Titsias' collapsed bound over inducing points Z (M, d) for a grid of length scales.
//
// 1. gpz_gene_kernel_project_sparse:  out[l, g, m] = sum_{stored (g, n)} v_gn k_l(z_m, x_n),  fp64 (n_ell, D, M) -- K_zx Y^T of
//    every gene of a whole data set stored as its non-zeros (the by-gene arrays of gene_rows.h), for every length scale, with
//    K_zx generated from the fp64 coordinates (cov.h, CovF64: the bits gram.hip sums into K_zx K_xz) and never stored.
//    A workgroup of GR_THREADS threads owns (gene, chunk of its row, block of GR_THREADS inducing points); thread t holds
//    z_m of its inducing point and n_ell accumulators in registers.  The row is swept GR_THREADS entries at a time: every
//    thread stages one entry (value, coordinates of its spot) in LDS, then every thread walks the staged entries in their
//    order (an LDS broadcast each): the distance of the pair once, its n_ell covariances, n_ell multiply-adds.  The cost is
//    the n_ell exp per (entry, inducing point); the reads are the row once per block of inducing points.
//    A row longer than the plan's chunk (a multiple of GR_THREADS, at least N / 4: at most GP_MAX_CHUNKS per row) is cut
//    into chunks of that many entries, one workgroup each; chunk 0 goes to `out`, chunk c >= 1 of a gene whose row starts
//    at entry lo to slot lo / chunk + c - 1 of `partials` (the slots of different genes cannot meet: lo / chunk +
//    ceil(len / chunk) <= (lo + len) / chunk + 1; nnz / chunk + 1 slots of n_ell x M values), and gp_fold_kernel adds the
//    slots of a gene to `out` in ascending order.  A sum is therefore: the entries of a chunk in row order, sequentially,
//    each term the rounded product v k added to the running sum; then the chunks in order.  It depends on the plan's chunk
//    (a function of N alone) and on nothing else: not on the grid, not on the workgroup.  No atomics.
//
//    The plan also says which way is faster (generate): generating costs c = 0.98 ps per (entry, inducing point, length scale)
//    on an MI355X, the fp64 vector rate at about 38 operations per exp; filling a K_xz per length scale (gpz_kfill) and
//    gathering its rows (gpz_counts_matmul) costs a = 38 ps per element of K_xz and b = 0.85 ps per (entry, inducing point,
//    length scale) (D = 17 702, N = 39 694, M = 256, 8 length scales, 1 % and 5 % stored).  Generating wins while
//    nnz (c - b) < N a, i.e. below N a / (c - b) = 290 N stored entries; above it gene_spatial_gp composes the other two.
//
// 2. gpz_gene_gp_profile: per (gene, length scale) the maximum over t = log delta, delta = tau / s, of the bound with s
//    profiled out.  With B = Phi Phi^T = U diag(lam) U^T, p = U^T Phi y, c = N - sum lam:
//      Q(delta) = y.y - sum_i p_i^2 / (delta + lam_i),    R = Q / delta,    s = R / N,    tau = s delta,
//      F(t) = -1/2 [ N log 2 pi + N log(R / N) + N + (N - M) t + sum_i log(delta + lam_i) + c / delta ],
//      g(t) = -2 dF/dt = N delta S2 / Q - sum_i lam_i / (delta + lam_i) - c / delta,       S_k = sum_i p_i^2 / (delta + lam_i)^k,
//      dg/dt = N [ delta S2 / Q - 2 delta^2 S3 / Q - (delta S2 / Q)^2 ] + delta sum_i lam_i / (delta + lam_i)^2 + c / delta.
//    F is evaluated on a uniform grid of GPP_GRID points over [log delta_min, log delta_max] (F need not be unimodal); the
//    best point, ties to the lower index, starts the refinement between its two grid neighbours: Newton steps on g in t
//    kept inside a bracket (g < 0 at its lower end once seen, g > 0 at its upper end), bisecting whenever the step leaves
//    the bracket, the slope is not positive or the last Newton step did not halve |g| -- gene_dispersion.hip's solver.
//    It stops at a step or bracket <= GPP_TOL_T.  When the best grid point is the first and g >= 0 there, the optimum is
//    the lower bound (status 2); when it is the last and g <= 0 there, no spatial variance shows in range (status 1).
//    y.y <= 0 (or not finite), or Q <= 0 or F not finite at a grid point: degenerate (status 3, NaN).
//    One wave per pair; lane j owns the terms j, j + 64, ... and the 64 partial sums are added in a fixed binary tree.
//
// fp64 throughout; two calls agree bit for bit.  Built with -ffp-contract=off: the sums are those of the same expressions in
// numpy, each product and sum rounded on its own (cov.h writes the fused multiply-adds of the covariance out).
#include "cov.h"
#include "gene_rows.h"

namespace gpz {
namespace grk {

constexpr int GP_MAX_M = 1024;
constexpr int GP_MAX_L = 16;
constexpr int GP_MAX_CHUNKS = 4;       // chunks a row is cut into at most
constexpr int64_t GP_GATHER_PER_SPOT = 290;   // stored entries per spot above which a stored K_xz, gathered, is faster (below)
constexpr int GP_WG = 32768;           // workgroups along the genes: one gene each up to here, the hardware deals them out

struct GpArgs {
  GrRows r;
  const double* X;
  const double* Z;
  const double* ell;
  double* out;
  double* partials;
  int64_t M, chunk;
  int d, nl;
};

__device__ inline int64_t gp_chunks(int64_t len, int64_t chunk) { return len <= chunk ? 1 : (len + chunk - 1) / chunk; }

template <int KIND>
__global__ __launch_bounds__(GR_THREADS) void gp_project_kernel(const GpArgs a) {
  using Cov = CovF64<KIND>;
  __shared__ double sx[GR_THREADS][4];
  __shared__ double sv[GR_THREADS];
  __shared__ double scf[GP_MAX_L];
  const int tid = threadIdx.x;
  const int64_t m = int64_t(blockIdx.z) * GR_THREADS + tid;
  const int64_t c = blockIdx.y;
  const bool low_d = a.d <= 2;
  const int nl = a.nl;
  if (tid < GP_MAX_L) scf[tid] = tid < nl ? Cov::coef(a.ell[tid]) : 0.0;
  double z[4] = {0.0, 0.0, 0.0, 0.0};
  if (m < a.M) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < a.d) z[k] = a.Z[m * a.d + k];
  }
  for (int64_t g = blockIdx.x; g < a.r.D; g += gridDim.x) {
    int64_t lo, hi;
    gr_row(a.r, g, lo, hi);
    if (c >= gp_chunks(hi - lo, a.chunk)) continue;              // chunk 0 exists for an empty row too: it writes the zeros
    const int64_t c_lo = lo + c * a.chunk;
    const int64_t c_hi = c_lo + a.chunk < hi ? c_lo + a.chunk : hi;
    double acc[GP_MAX_L];
#pragma unroll
    for (int l = 0; l < GP_MAX_L; ++l) acc[l] = 0.0;
    for (int64_t s0 = c_lo; s0 < c_hi; s0 += GR_THREADS) {
      __syncthreads();                                           // the last sweep's readers are done (and scf is written)
      {
        const int64_t k = s0 + tid;
        int32_t spot = 0;
        float x = 0.f;
        const bool ok = k < c_hi && gr_entry(a.r, k, spot, x);   // an entry out of range counts as a stored zero
        sv[tid] = ok ? double(x) : 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) sx[tid][q] = (ok && q < a.d) ? a.X[int64_t(spot) * a.d + q] : 0.0;
      }
      __syncthreads();
      const int ne = int(c_hi - s0 < GR_THREADS ? c_hi - s0 : GR_THREADS);
      if (m < a.M) {
        for (int e = 0; e < ne; ++e) {
          const double rad = Cov::radial(z, sx[e], low_d);
          const double v = sv[e];
#pragma unroll
          for (int l = 0; l < GP_MAX_L; ++l)
            if (l < nl) acc[l] += v * Cov::unit(scf[l], rad);
        }
      }
    }
    if (m < a.M) {
      double* const dst = c == 0 ? a.out + g * a.M + m : a.partials + (lo / a.chunk + c - 1) * nl * a.M + m;
      const int64_t stride = c == 0 ? a.r.D * a.M : a.M;
#pragma unroll
      for (int l = 0; l < GP_MAX_L; ++l)
        if (l < nl) dst[l * stride] = acc[l];
    }
  }
}

// out[l, g, m] += the slots of gene g in ascending chunk order
__global__ __launch_bounds__(GR_THREADS) void gp_fold_kernel(const GpArgs a) {
  const int64_t per_gene = int64_t(a.nl) * a.M;
  const int64_t total = a.r.D * per_gene;
  const int64_t stride = int64_t(gridDim.x) * GR_THREADS;
  for (int64_t e = int64_t(blockIdx.x) * GR_THREADS + threadIdx.x; e < total; e += stride) {
    const int64_t g = e / per_gene, lm = e - g * per_gene;
    int64_t lo, hi;
    gr_row(a.r, g, lo, hi);
    const int64_t nc = gp_chunks(hi - lo, a.chunk);
    if (nc <= 1) continue;
    const int64_t l = lm / a.M, m = lm - l * a.M;
    double* const o = a.out + (l * a.r.D + g) * a.M + m;
    double v = *o;
    for (int64_t c = 1; c < nc; ++c) v += a.partials[(lo / a.chunk + c - 1) * per_gene + lm];
    *o = v;
  }
}

struct GpPlan {
  int64_t chunk, slots;
  int workgroups, m_blocks, chunks, generate;
  size_t bytes;
};

static GpPlan gp_plan(int64_t N, int64_t D, int64_t nnz, int64_t M, int nl) {
  GpPlan p{};
  const int64_t quarter = (N + GP_MAX_CHUNKS - 1) / GP_MAX_CHUNKS;
  p.chunk = (quarter + GR_THREADS - 1) / GR_THREADS * GR_THREADS;
  p.chunks = int((N + p.chunk - 1) / p.chunk);                   // a row has at most N entries
  p.slots = nnz / p.chunk + 1;
  p.workgroups = int(D < GP_WG ? D : GP_WG);
  p.m_blocks = int((M + GR_THREADS - 1) / GR_THREADS);
  p.generate = nnz <= GP_GATHER_PER_SPOT * N ? 1 : 0;
  Carver c(nullptr);
  c.take<double>(size_t(p.slots) * nl * M);
  p.bytes = c.used();
  return p;
}

static int gp_check_shape(const char* who, int64_t N, int64_t D, int64_t nnz, int64_t M, int nl) {
  if (int rc = gr_check_shape(who, N, D, nnz)) return rc;
  GPZ_REQUIRE(M >= 1 && M <= GP_MAX_M, "%s: M = %lld inducing points unsupported (1..%d)", who, (long long)M, GP_MAX_M);
  GPZ_REQUIRE(nl >= 1 && nl <= GP_MAX_L, "%s: n_ell = %d length scales unsupported (1..%d)", who, nl, GP_MAX_L);
  return 0;
}

// ---- the profile ----------------------------------------------------------------------------------------------------------

constexpr int GPP_THREADS = 64;        // one wave per (gene, length scale)
constexpr int GPP_GRID = 33;
constexpr double GPP_TOL_T = 1e-9;
constexpr int GPP_MAX_ITER = 100;
constexpr int GPP_WG = 8192;

template <int NV>
__device__ inline void gpp_tree(double (*red)[GPP_THREADS]) {
  __syncthreads();
  for (int h = GPP_THREADS / 2; h >= 1; h >>= 1) {
    if (int(threadIdx.x) < h)
      for (int v = 0; v < NV; ++v) red[v][threadIdx.x] += red[v][threadIdx.x + h];
    __syncthreads();
  }
}

struct GppEval { double F, Q, g, dg; };

__global__ __launch_bounds__(GPP_THREADS) void gp_profile_kernel(const double* __restrict__ p, const double* __restrict__ lam,
                                                                 const double* __restrict__ yty, double Nd, int64_t D, int64_t M, int nl,
                                                                 double t_lo, double t_hi, double* __restrict__ loglik,
                                                                 double* __restrict__ delta, double* __restrict__ s2,
                                                                 double* __restrict__ tau2, int32_t* __restrict__ status,
                                                                 int32_t* __restrict__ iterations) {
  __shared__ double sq[GP_MAX_M], sl[GP_MAX_M];
  __shared__ double red[6][GPP_THREADS];
  const int tid = threadIdx.x;
  const double Md = double(M);
  const double step = (t_hi - t_lo) / (GPP_GRID - 1);
  auto t_at = [&](int i) { return i == GPP_GRID - 1 ? t_hi : t_lo + i * step; };
  for (int64_t pair = blockIdx.x; pair < D * nl; pair += gridDim.x) {
    const int64_t g = pair / nl, l = pair - g * nl;
    const double* const pp = p + (l * D + g) * M;
    const double* const pl = lam + l * M;
    __syncthreads();                                             // the last pair's readers are done
    double lsum = 0.0;
    for (int64_t i = tid; i < M; i += GPP_THREADS) {
      const double q = pp[i], w = pl[i];
      sq[i] = q * q;
      sl[i] = w;
      lsum += w;
    }
    red[0][tid] = lsum;
    gpp_tree<1>(red);
    const double c = Nd - red[0][0];
    const double yy = yty[g];
    __syncthreads();

    auto eval = [&](double t) {
      const double dl = exp(t);
      double s1 = 0.0, s2_ = 0.0, s3 = 0.0, l1 = 0.0, l2 = 0.0, lg = 0.0;
      for (int64_t i = tid; i < M; i += GPP_THREADS) {
        const double den = dl + sl[i], w = 1.0 / den, qw = sq[i] * w, lw = sl[i] * w;
        s1 += qw;
        s2_ += qw * w;
        s3 += qw * w * w;
        l1 += lw;
        l2 += lw * w;
        lg += log(den);
      }
      red[0][tid] = s1;
      red[1][tid] = s2_;
      red[2][tid] = s3;
      red[3][tid] = l1;
      red[4][tid] = l2;
      red[5][tid] = lg;
      gpp_tree<6>(red);
      s1 = red[0][0];
      s2_ = red[1][0];
      s3 = red[2][0];
      l1 = red[3][0];
      l2 = red[4][0];
      lg = red[5][0];
      __syncthreads();
      GppEval e;
      e.Q = yy - s1;
      e.F = -0.5 * (Nd * 1.8378770664093454836 + Nd * log(e.Q / (dl * Nd)) + Nd + (Nd - Md) * t + lg + c / dl);
      const double u = dl * s2_ / e.Q;
      e.g = Nd * u - l1 - c / dl;
      e.dg = Nd * (u - 2.0 * dl * dl * s3 / e.Q - u * u) + dl * l2 + c / dl;
      return e;
    };

    int st = 3, it = 0;
    double t_out = double(NAN);
    bool bad = !(yy > 0.0) || yy > 1.7e308;
    if (!bad) {
      double best = -INFINITY;
      int bi = 0;
      for (int i = 0; i < GPP_GRID; ++i) {
        const GppEval e = eval(t_at(i));
        if (!(e.Q > 0.0) || !(fabs(e.F) <= 1.7e308)) bad = true;
        if (e.F > best) {
          best = e.F;
          bi = i;
        }
      }
      if (!bad) {
        double blo = t_at(bi > 0 ? bi - 1 : 0), bhi = t_at(bi < GPP_GRID - 1 ? bi + 1 : GPP_GRID - 1);
        double t = t_at(bi), prev = double(INFINITY);
        bool stepped = false;
        st = 0;
        while (it < GPP_MAX_ITER) {
          const GppEval e = eval(t);
          ++it;
          if (it == 1 && bi == 0 && e.g >= 0.0) {                // F falls from the lower bound on
            st = 2;
            break;
          }
          if (it == 1 && bi == GPP_GRID - 1 && e.g <= 0.0) {     // F still rises at the upper bound
            st = 1;
            break;
          }
          if (e.g < 0.0) blo = t;
          else if (e.g > 0.0) bhi = t;
          else break;
          const double tn = t - e.g / e.dg;
          if (e.dg > 0.0 && fabs(tn - t) <= GPP_TOL_T) {
            if (tn > blo && tn < bhi) t = tn;
            break;
          }
          const bool newton = !(stepped && fabs(e.g) > 0.5 * prev) && e.dg > 0.0 && tn > blo && tn < bhi;
          const double next = newton ? tn : 0.5 * (blo + bhi);
          stepped = newton;
          prev = fabs(e.g);
          const double moved = fabs(next - t);
          t = next;
          if (moved <= GPP_TOL_T || bhi - blo <= GPP_TOL_T) break;
        }
        t_out = t;
      }
    }
    double F_out = double(NAN), d_out = double(NAN), s_out = double(NAN);
    if (!bad) {
      const GppEval e = eval(t_out);
      d_out = exp(t_out);
      F_out = e.F;
      s_out = e.Q / (d_out * Nd);
    }
    if (tid == 0) {
      const int64_t o = g * nl + l;
      loglik[o] = F_out;
      delta[o] = d_out;
      s2[o] = s_out;
      tau2[o] = s_out * d_out;
      status[o] = st;
      iterations[o] = it;
    }
  }
}

static int gpp_check_shape(const char* who, int64_t D, int64_t M, int nl) {
  GPZ_REQUIRE(D >= 1 && D < (1ll << 31), "%s: D = %lld genes unsupported (1 <= D < 2^31)", who, (long long)D);
  GPZ_REQUIRE(M >= 1 && M <= GP_MAX_M, "%s: M = %lld inducing points unsupported (1..%d)", who, (long long)M, GP_MAX_M);
  GPZ_REQUIRE(nl >= 1 && nl <= GP_MAX_L, "%s: n_ell = %d length scales unsupported (1..%d)", who, nl, GP_MAX_L);
  return 0;
}

}  // namespace grk
}  // namespace gpz

using namespace gpz;
using namespace gpz::grk;

extern "C" int gpz_gene_kernel_project_sparse_plan(int64_t N, int64_t D, int64_t nnz, int64_t M, int32_t n_ell, int32_t* gene_chunk,
                                                   int32_t* workgroups, int32_t* generate, int64_t* partials_bytes) {
  if (int rc = gp_check_shape("gpz_gene_kernel_project_sparse", N, D, nnz, M, n_ell)) return rc;
  const GpPlan p = gp_plan(N, D, nnz, M, n_ell);
  if (gene_chunk) *gene_chunk = int32_t(p.chunk);
  if (workgroups) *workgroups = p.workgroups;
  if (generate) *generate = p.generate;
  if (partials_bytes) *partials_bytes = int64_t(p.bytes);
  return 0;
}

extern "C" int gpz_gene_kernel_project_sparse(const int64_t* row_ptr, const int32_t* row_spot, const int32_t* row_perm,
                                              const float* col_val, const double* X, const double* Z, const double* lengthscales,
                                              int64_t N, int64_t D, int64_t nnz, int64_t M, int32_t d, int32_t n_ell, int32_t kind,
                                              int32_t workgroups, double* out, void* partials, size_t partials_bytes,
                                              void* stream) {
  const char* who = "gpz_gene_kernel_project_sparse";
  GPZ_REQUIRE(row_ptr && X && Z && lengthscales && out && partials, "%s: null pointer", who);
  if (int rc = gp_check_shape(who, N, D, nnz, M, n_ell)) return rc;
  GPZ_REQUIRE(nnz == 0 || (row_spot && row_perm && col_val), "%s: null pointer (non-zeros)", who);
  GPZ_REQUIRE(d >= 1 && d <= 4, "%s: input dimension %d unsupported (1..4)", who, d);
  GPZ_REQUIRE(kind == GPZ_KERNEL_RBF || kind == GPZ_KERNEL_MATERN32 || kind == GPZ_KERNEL_MATERN12 || kind == GPZ_KERNEL_MATERN52,
              "%s: kernel kind %d unsupported (stationary kinds 0, 1, 4, 5)", who, kind);
  GPZ_REQUIRE(workgroups >= 0 && workgroups <= 65535, "%s: workgroups = %d outside [0, 65535] (0: the plan's)", who, workgroups);
  GPZ_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 15) == 0, "%s: partials must be 16-byte aligned", who);
  const GpPlan p = gp_plan(N, D, nnz, M, n_ell);
  GPZ_REQUIRE(partials_bytes >= p.bytes, "%s: partials too small (%zu bytes, %zu needed)", who, partials_bytes, p.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  Carver c(partials);
  GpArgs a;
  a.r = GrRows{row_ptr, row_spot, row_perm, col_val, N, D, nnz};
  a.X = X;
  a.Z = Z;
  a.ell = lengthscales;
  a.out = out;
  a.partials = c.take<double>(size_t(p.slots) * n_ell * M);
  a.M = M;
  a.chunk = p.chunk;
  a.d = d;
  a.nl = n_ell;
  const dim3 grid(unsigned(workgroups ? workgroups : p.workgroups), unsigned(p.chunks), unsigned(p.m_blocks));
  switch (kind) {
    case GPZ_KERNEL_RBF: hipLaunchKernelGGL(gp_project_kernel<0>, grid, dim3(GR_THREADS), 0, s, a); break;
    case GPZ_KERNEL_MATERN32: hipLaunchKernelGGL(gp_project_kernel<1>, grid, dim3(GR_THREADS), 0, s, a); break;
    case GPZ_KERNEL_MATERN12: hipLaunchKernelGGL(gp_project_kernel<4>, grid, dim3(GR_THREADS), 0, s, a); break;
    default: hipLaunchKernelGGL(gp_project_kernel<5>, grid, dim3(GR_THREADS), 0, s, a); break;
  }
  GPZ_LAUNCH_OK();
  if (p.chunks > 1) {
    int64_t blocks = (D * n_ell * M + GR_THREADS - 1) / GR_THREADS;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(gp_fold_kernel, dim3(unsigned(blocks)), dim3(GR_THREADS), 0, s, a);
    GPZ_LAUNCH_OK();
  }
  return 0;
}

extern "C" int gpz_gene_gp_profile_plan(int64_t D, int64_t M, int32_t n_ell, int32_t* grid_points, int32_t* workgroups,
                                        double* tol_t, int32_t* max_iter) {
  if (int rc = gpp_check_shape("gpz_gene_gp_profile", D, M, n_ell)) return rc;
  const int64_t pairs = D * n_ell;
  if (grid_points) *grid_points = GPP_GRID;
  if (workgroups) *workgroups = int32_t(pairs < GPP_WG ? pairs : GPP_WG);
  if (tol_t) *tol_t = GPP_TOL_T;
  if (max_iter) *max_iter = GPP_MAX_ITER;
  return 0;
}

extern "C" int gpz_gene_gp_profile(const double* p, const double* lam, const double* yty, int64_t N, int64_t D, int64_t M,
                                   int32_t n_ell, double delta_min, double delta_max, double* loglik, double* delta, double* s2,
                                   double* tau2, int32_t* status, int32_t* iterations, void* stream) {
  const char* who = "gpz_gene_gp_profile";
  GPZ_REQUIRE(p && lam && yty && loglik && delta && s2 && tau2 && status && iterations, "%s: null pointer", who);
  if (int rc = gpp_check_shape(who, D, M, n_ell)) return rc;
  GPZ_REQUIRE(N >= 2 && N < (1ll << 31), "%s: N = %lld spots unsupported (2 <= N < 2^31)", who, (long long)N);
  GPZ_REQUIRE(delta_min > 0.0 && delta_min < delta_max && delta_max <= 1.7e308,
              "%s: delta range (%g, %g) unsupported (0 < delta_min < delta_max, both finite)", who, delta_min, delta_max);
  const int64_t pairs = D * n_ell;
  const unsigned grid = unsigned(pairs < GPP_WG ? pairs : GPP_WG);
  hipLaunchKernelGGL(gp_profile_kernel, dim3(grid), dim3(GPP_THREADS), 0, static_cast<hipStream_t>(stream), p, lam, yty, double(N), D,
                     M, int(n_ell), log(delta_min), log(delta_max), loglik, delta, s2, tau2, status, iterations);
  GPZ_LAUNCH_OK();
  return 0;
}
