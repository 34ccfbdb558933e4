// gene_dispersion.hip -- the maximum-likelihood negative-binomial inverse dispersion theta of every gene of a whole data set
// stored as its non-zeros, under the constant-rate null of gpz_gene_deviance_sparse: mu_n = p size_n, p = sum_n y_n / sum_n
// size_n (edgeR / DESeq2 / glmGamPoi's gene-wise overdispersion MLE with the rate held at the null).  Per gene it returns
// theta, the gain in log-likelihood over the Poisson limit and the Poisson log-likelihood: which genes are overdispersed at
// all, and where theta should start for each of them.
//
// With t = log theta, x_n = mu_n / theta and integer counts y the score in t is
//   S(t) = sum_{all n} a_n + sum_{stored} b_n,     a_n = theta h(x_n),  h(x) = x / (1 + x) - log1p(x)   (<= 0)
//                                                  b_n = theta sum_{k < y} (mu_n - k) / ((theta + k)(theta + mu_n))
//   gain(theta) = l(theta) - l(inf) = sum_{all n} theta (x_n - log1p(x_n)) + sum_{stored} sum_{k < y} log((theta + k) / (theta + mu_n))
//   poisson_loglik = sum_{stored} [ y log mu_n - lgamma(y + 1) ] - sum_n y_n
// and no term is formed as a difference of large numbers:
//   * h(x) and x - log1p(x) for x <= 1/2 from log1p(x) = 2 atanh(s), s = x / (2 + x):
//       h(x) = -x^2 / ((1 + x)(2 + x)) - 2 s^3 P(s^2),   x - log1p(x) = s x - 2 s^3 P(s^2),   P(z) = 1/3 + z/5 + z^2/7 + ...
//     (both terms of h have one sign; 12 terms of P leave 0.04^12 / 27); above 1/2 the plain expressions lose one digit.
//   * the k-sums explicitly for k < GD_M = 16; for a count above 16 the rest is the difference of the asymptotic series of
//     psi (lgamma) at M = theta + 16 and X = theta + y, both >= 16, with the logarithms combined first: u = (y - 16) / M,
//       sum_{16 <= k < y} [1 / (theta + k) - 1 / (theta + mu)]
//           = [log1p(u) - u] + (y - 16)(mu - 16) / (M (theta + mu)) + (y - 16) / (2 M X) + ser(M) - ser(X)        (u <= 1/2)
//       sum_{16 <= k < y} log((theta + k) / (theta + mu))
//           = M [log1p(u) - u] - log1p(u) / 2 + (y - 16) log((theta + y) / (theta + mu)) + sr(X) - sr(M)
//     so at theta = 1e6 the terms are of the size of the result, y^2 / theta, not of y.  (The plain psi(y + theta) -
//     psi(theta) loses theta / y digits there.)  log((theta + k) / (theta + mu)) is log1p of (k - mu) / (theta + mu) where
//     that is at most 1/2 in size and the logarithm of the quotient elsewhere.
//
// Root: S(-inf) = the number of stored entries > 0, and S changes sign at most once on the data this is meant for; the
// solver keeps a bracket [lo, hi] in t with S(lo) > 0 > S(hi).  S(log theta_max) >= 0: no overdispersion in range, theta =
// +inf, gain 0 (status 1).  S(log theta_min) <= 0: theta_min (status 2).  Otherwise it starts from the moment estimate
//   theta_0 = sum_n mu_n^2 / ( sum_n (y_n - mu_n)^2 - sum_n y_n ),   theta_max where the denominator is <= 0,
// clipped into [theta_min, theta_max] (Var y = mu + mu^2 / theta summed over the spots), and takes Newton steps in t with
// dS/dt summed beside S (the derivative needs few digits and is formed plainly), bisecting instead whenever the step leaves
// the bracket, the slope is not negative, or the last Newton step did not halve |S|.  It stops when the step (Newton's, also
// where rounding puts it on the bracket's end, or the bisection's) or the bracket is <= GD_TOL_T; the returned t is the last
// iterate, which lies inside the bracket or is its end.  Every loop is bounded: max_iter <= 200
// evaluations, GD_M explicit terms per entry, N / GR_THREADS spots per thread.
//
// One workgroup of GR_THREADS threads per gene at a time, genes dealt to a fixed number of workgroups in a fixed order, and
// every sum in the fixed order of gene_rows.h: a gene's result depends on neither the grid nor the workgroup and two calls
// agree bit for bit.  Each evaluation sweeps the N sizes (fp64, 8 N bytes: they stay in L2) and the gene's stored entries;
// when all sizes are equal (found once per call, with sum size and sum size^2) the all-spot sums are N f(x) and the sweep
// is skipped.  The decisions of the solver are taken from the reduced sums, which every thread reads alike, so the
// workgroup never diverges at a barrier.  Nothing of D x N or nnz elements is allocated; the scratch is four fp64 words.
//
// Built with -ffp-contract=off, like gene_rank.hip: the terms are those of the same expressions written in numpy.
#include "gene_rows.h"

namespace gpz {
namespace grk {

constexpr int GD_WG = 2048;            // workgroups (eight per CU, a full CU of waves)
constexpr int GD_M = 16;               // explicit k-terms per stored entry; above it the series' difference
constexpr double GD_TOL_T = 1e-9;      // the solver stops at a step or bracket of this size in t = log theta
constexpr int GD_MAX_ITER = 200;
constexpr float GD_VALUE_LIMIT = 16777216.f;      // 2^24: counts are exact in fp32 below it

// P(z) = 1/3 + z/5 + z^2/7 + ... + z^11/25
__device__ inline double gd_atanh_tail(double z) {
  double p = 1.0 / 25;
  for (int j = 23; j >= 3; j -= 2) p = p * z + 1.0 / j;
  return p;
}

// x - log1p(x), x >= 0
__device__ inline double gd_xml(double x) {
  if (x <= 0.5) {
    const double s = x / (2.0 + x);
    return s * x - 2.0 * (s * s * s) * gd_atanh_tail(s * s);
  }
  return x - log1p(x);
}

// h(x) = x / (1 + x) - log1p(x), x >= 0
__device__ inline double gd_h(double x) {
  if (x <= 0.5) {
    const double s = x / (2.0 + x);
    return -(x * x) / ((1.0 + x) * (2.0 + x)) - 2.0 * (s * s * s) * gd_atanh_tail(s * s);
  }
  return x / (1.0 + x) - log1p(x);
}

// psi(x) = log x - 1 / (2 x) - gd_psi_ser(x);  lgamma(x) = (x - 1/2) log x - x + log(2 pi) / 2 + gd_lgamma_ser(x);  x >= 16
__device__ inline double gd_psi_ser(double x) {
  const double i = 1.0 / x, i2 = i * i;
  return i2 * (1.0 / 12 - i2 * (1.0 / 120 - i2 * (1.0 / 252 - i2 * (1.0 / 240 - i2 * (1.0 / 132 - i2 * (691.0 / 32760 - i2 / 12))))));
}

__device__ inline double gd_lgamma_ser(double x) {
  const double i = 1.0 / x, i2 = i * i;
  return i * (1.0 / 12 - i2 * (1.0 / 360 - i2 * (1.0 / 1260 - i2 * (1.0 / 1680 - i2 * (1.0 / 1188 - i2 * (691.0 / 360360))))));
}

// psi'(x), x >= 16, to the few digits the Newton slope needs
__device__ inline double gd_trigamma(double x) {
  const double i = 1.0 / x, i2 = i * i;
  return i + 0.5 * i2 + i * i2 * (1.0 / 6 - i2 * (1.0 / 30 - i2 / 42));
}

// log((theta + k) / (theta + mu)) with itm = 1 / (theta + mu)
__device__ inline double gd_log_ratio(double th, double k, double mu, double itm) {
  const double arg = (k - mu) * itm;
  return fabs(arg) <= 0.5 ? log1p(arg) : log((th + k) * itm);
}

// b = theta sum_{k < y} (mu - k) / ((theta + k)(theta + mu)) and db/dt = b + theta^2 sum_{k < y} [1 / (theta + mu)^2 - 1 / (theta + k)^2]
__device__ inline void gd_entry_score(double y, int yi, double mu, double th, double& b, double& db) {
  const double tm = th + mu, itm = 1.0 / tm;
  const int ke = yi < GD_M ? yi : GD_M;
  double s = 0.0, q = 0.0;
  for (int k = 0; k < ke; ++k) {
    const double kd = double(k), rk = 1.0 / (th + kd);
    s += (mu - kd) * rk;
    q += (kd - mu) * (2.0 * th + kd + mu) * (rk * rk);
  }
  double c = s * itm, e = q * (itm * itm);
  if (yi > GD_M) {
    const double M = th + GD_M, X = th + y, rest = y - GD_M, u = rest / M;
    c += (u <= 0.5 ? rest * (mu - GD_M) / (M * tm) - gd_xml(u) : log1p(u) - rest * itm) + 0.5 * rest / (M * X) +
         (gd_psi_ser(M) - gd_psi_ser(X));
    e += rest * (itm * itm) - (gd_trigamma(M) - gd_trigamma(X));
  }
  b = th * c;
  db = b + (th * th) * e;
}

// sum_{k < y} log((theta + k) / (theta + mu))
__device__ inline double gd_entry_gain(double y, int yi, double mu, double th) {
  const double itm = 1.0 / (th + mu);
  const int ke = yi < GD_M ? yi : GD_M;
  double v = 0.0;
  for (int k = 0; k < ke; ++k) v += gd_log_ratio(th, double(k), mu, itm);
  if (yi > GD_M) {
    const double M = th + GD_M, X = th + y, rest = y - GD_M, u = rest / M;
    v += -M * gd_xml(u) - 0.5 * log1p(u) + rest * gd_log_ratio(th, y, mu, itm) + (gd_lgamma_ser(X) - gd_lgamma_ser(M));
  }
  return v;
}

// a stored entry that counts: a non-negative integer below 2^24 (anything else raises `bad`), not zero, at a spot of
// positive size (a stored count at a spot of size <= 0 raises `bad` too)
__device__ inline bool gd_entry(const GrRows& r, const double* __restrict__ size, int64_t k, double& y, int& yi, double& sz,
                                int& bad) {
  int32_t spot;
  float x;
  if (!gr_entry(r, k, spot, x)) return false;
  if (!(x >= 0.f) || x != floorf(x) || x >= GD_VALUE_LIMIT) {
    bad |= 1;
    return false;
  }
  if (x == 0.f) return false;
  sz = size[spot];
  if (!(sz > 0.0) || sz > 1.7e308) {
    bad |= 2;
    return false;
  }
  y = double(x);
  yi = int(x);
  return true;
}

// totals[0] = sum size, [1] = sum size^2, [2] = 1 when all sizes are equal (and positive), [3] = that size; a negative or
// non-finite size raises info
__global__ __launch_bounds__(GR_THREADS) void gd_total_kernel(const double* __restrict__ size, int64_t N, double* __restrict__ totals,
                                                              int32_t* __restrict__ info) {
  __shared__ double red[4][GR_THREADS];
  double a = 0.0, a2 = 0.0, mn = INFINITY, mx = -INFINITY;
  bool bad = false;
  for (int64_t n = threadIdx.x; n < N; n += GR_THREADS) {
    const double s = size[n];
    if (!(s >= 0.0) || s > 1.7e308) {
      bad = true;
      continue;
    }
    a += s;
    a2 += s * s;
    mn = s < mn ? s : mn;
    mx = s > mx ? s : mx;
  }
  if (bad) atomicOr(info, 2);
  red[0][threadIdx.x] = a;
  red[1][threadIdx.x] = a2;
  red[2][threadIdx.x] = mn;
  red[3][threadIdx.x] = mx;
  __syncthreads();
  for (int h = GR_THREADS / 2; h >= 1; h >>= 1) {
    if (int(threadIdx.x) < h) {
      red[0][threadIdx.x] += red[0][threadIdx.x + h];
      red[1][threadIdx.x] += red[1][threadIdx.x + h];
      const double l2 = red[2][threadIdx.x + h], h2 = red[3][threadIdx.x + h];
      if (l2 < red[2][threadIdx.x]) red[2][threadIdx.x] = l2;
      if (h2 > red[3][threadIdx.x]) red[3][threadIdx.x] = h2;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    totals[0] = red[0][0];
    totals[1] = red[1][0];
    totals[2] = (red[2][0] == red[3][0] && red[2][0] > 0.0) ? 1.0 : 0.0;
    totals[3] = red[2][0];
  }
}

__global__ __launch_bounds__(GR_THREADS) void gd_kernel(GrRows r, const double* __restrict__ size, const double* __restrict__ totals,
                                                        double theta_min, double theta_max, int max_iter,
                                                        double* __restrict__ theta, double* __restrict__ gain,
                                                        double* __restrict__ poisson_loglik, int32_t* __restrict__ status,
                                                        int32_t* __restrict__ iterations, int32_t* __restrict__ info) {
  __shared__ double red[4][GR_THREADS];
  const int64_t N = r.N;
  const double Nd = double(N);
  const double Stot = totals[0], S2 = totals[1], c0 = totals[3];
  const bool equal = totals[2] != 0.0;
  const double t_min = log(theta_min), t_max = log(theta_max);
  int bad = 0;
  for (int64_t d = blockIdx.x; d < r.D; d += gridDim.x) {
    int64_t lo, hi;
    gr_row(r, d, lo, hi);
    // the sums that do not depend on theta: sum y, sum y^2, sum y size, sum [ y log size - lgamma(y + 1) ]
    double sy = 0.0, syy = 0.0, sys = 0.0, sl = 0.0;
    for (int64_t k = lo + threadIdx.x; k < hi; k += GR_THREADS) {
      double y, sz;
      int yi;
      if (!gd_entry(r, size, k, y, yi, sz, bad)) continue;
      sy += y;
      syy += y * y;
      sys += y * sz;
      sl += y * log(sz) - lgamma(y + 1.0);
    }
    red[0][threadIdx.x] = sy;
    red[1][threadIdx.x] = syy;
    red[2][threadIdx.x] = sys;
    red[3][threadIdx.x] = sl;
    gr_tree<4>(red);
    sy = red[0][0];
    syy = red[1][0];
    sys = red[2][0];
    sl = red[3][0];
    __syncthreads();
    if (!(sy > 0.0) || !(Stot > 0.0)) {                               // no counts
      if (threadIdx.x == 0) {
        theta[d] = double(NAN);
        gain[d] = 0.0;
        poisson_loglik[d] = 0.0;
        status[d] = 4;
        iterations[d] = 0;
      }
      continue;
    }
    const double p = sy / Stot;

    // S(t) and dS/dt at theta = th: the same values in every thread
    auto score = [&](double th, double& S, double& dS) {
      double a = 0.0, da = 0.0;
      if (equal) {
        if (threadIdx.x == 0) {
          const double x = p * c0 / th, hx = th * gd_h(x), q = x / (1.0 + x);
          a = Nd * hx;
          da = Nd * (hx + th * (q * q));
        }
      } else {
        for (int64_t n = threadIdx.x; n < N; n += GR_THREADS) {
          const double x = p * size[n] / th, hx = th * gd_h(x), q = x / (1.0 + x);
          a += hx;
          da += hx + th * (q * q);
        }
      }
      for (int64_t k = lo + threadIdx.x; k < hi; k += GR_THREADS) {
        double y, sz, b, db;
        int yi, ignore = 0;
        if (!gd_entry(r, size, k, y, yi, sz, ignore)) continue;
        gd_entry_score(y, yi, p * sz, th, b, db);
        a += b;
        da += db;
      }
      red[0][threadIdx.x] = a;
      red[1][threadIdx.x] = da;
      gr_tree<2>(red);
      S = red[0][0];
      dS = red[1][0];
      __syncthreads();
    };
    auto gain_at = [&](double th) {
      double g = 0.0;
      if (equal) {
        if (threadIdx.x == 0) g = Nd * (th * gd_xml(p * c0 / th));
      } else {
        for (int64_t n = threadIdx.x; n < N; n += GR_THREADS) g += th * gd_xml(p * size[n] / th);
      }
      for (int64_t k = lo + threadIdx.x; k < hi; k += GR_THREADS) {
        double y, sz;
        int yi, ignore = 0;
        if (!gd_entry(r, size, k, y, yi, sz, ignore)) continue;
        g += gd_entry_gain(y, yi, p * sz, th);
      }
      red[0][threadIdx.x] = g;
      gr_tree<1>(red);
      g = red[0][0];
      __syncthreads();
      return g;
    };

    double th_out, g_out = 0.0, S, dS;
    int st, it = 0;
    score(theta_max, S, dS);
    if (S >= 0.0) {
      th_out = double(INFINITY);
      st = 1;
    } else {
      score(theta_min, S, dS);
      if (S <= 0.0) {
        th_out = theta_min;
        st = 2;
      } else {
        // the moment start: sum (y - mu)^2 = sum y^2 - 2 p sum y size + p^2 sum size^2
        const double num = (p * p) * S2, den = (syy - 2.0 * p * sys + num) - sy;
        double th = den > 0.0 ? num / den : theta_max;
        th = th < theta_min ? theta_min : (th > theta_max ? theta_max : th);
        double t = log(th), blo = t_min, bhi = t_max, prev = double(INFINITY);
        bool stepped = false;                                         // the iterate came from a Newton step
        st = 3;
        while (it < max_iter) {
          score(th, S, dS);
          ++it;
          if (S > 0.0) blo = t;
          else if (S < 0.0) bhi = t;
          else {
            st = 0;
            break;
          }
          const double tn = t - S / dS;
          if (dS < 0.0 && fabs(tn - t) <= GD_TOL_T) {                   // a Newton step below the tolerance: taken where it
            if (tn > blo && tn < bhi) {                                 // stays inside the bracket, whose end t is otherwise
              t = tn;
              th = exp(t);
            }
            st = 0;
            break;
          }
          const bool newton = !(stepped && fabs(S) > 0.5 * prev) && dS < 0.0 && tn > blo && tn < bhi;
          const double next = newton ? tn : 0.5 * (blo + bhi);
          stepped = newton;
          prev = fabs(S);
          const double step = fabs(next - t);
          t = next;
          th = exp(t);
          if (step <= GD_TOL_T || bhi - blo <= GD_TOL_T) {
            st = 0;
            break;
          }
        }
        th_out = th;
      }
      g_out = gain_at(th_out);
    }
    if (threadIdx.x == 0) {
      theta[d] = th_out;
      gain[d] = g_out;
      poisson_loglik[d] = sl + sy * log(p) - sy;
      status[d] = st;
      iterations[d] = it;
    }
  }
  if (bad) atomicOr(info, bad);
}

struct GdPlan {
  double* totals;     // sum size, sum size^2, all-equal flag, the common size
  int workgroups;
  size_t bytes;
};

static GdPlan gd_plan(int64_t D, void* scratch) {
  Carver c(scratch);
  GdPlan p{};
  p.workgroups = int(D < GD_WG ? D : GD_WG);
  p.totals = c.take<double>(4);
  p.bytes = c.used();
  return p;
}

}  // namespace grk
}  // namespace gpz

using namespace gpz;
using namespace gpz::grk;

extern "C" int gpz_gene_dispersion_sparse_plan(int64_t N, int64_t D, int64_t nnz, int32_t* gene_chunk, int32_t* workgroups,
                                               double* tol_t, int64_t* partials_bytes) {
  if (int rc = gr_check_shape("gpz_gene_dispersion_sparse", N, D, nnz)) return rc;
  const GdPlan p = gd_plan(D, nullptr);
  if (gene_chunk) *gene_chunk = GR_THREADS;
  if (workgroups) *workgroups = p.workgroups;
  if (tol_t) *tol_t = GD_TOL_T;
  if (partials_bytes) *partials_bytes = int64_t(p.bytes);
  return 0;
}

extern "C" int gpz_gene_dispersion_sparse(const int64_t* row_ptr, const int32_t* row_spot, const int32_t* row_perm,
                                          const float* col_val, const double* size, int64_t N, int64_t D, int64_t nnz,
                                          double theta_min, double theta_max, int32_t max_iter, double* theta, double* gain,
                                          double* poisson_loglik, int32_t* status, int32_t* iterations, int32_t* info,
                                          void* partials, size_t partials_bytes, void* stream) {
  const char* who = "gpz_gene_dispersion_sparse";
  GPZ_REQUIRE(row_ptr && size && theta && gain && poisson_loglik && status && iterations && info && partials, "%s: null pointer",
              who);
  if (int rc = gr_check_shape(who, N, D, nnz)) return rc;
  GPZ_REQUIRE(nnz == 0 || (row_spot && row_perm && col_val), "%s: null pointer (non-zeros)", who);
  GPZ_REQUIRE(theta_min > 0.0 && theta_min < theta_max && theta_max <= 1.7e308,
              "%s: theta range (%g, %g) unsupported (0 < theta_min < theta_max, both finite)", who, theta_min, theta_max);
  GPZ_REQUIRE(max_iter >= 0 && max_iter <= GD_MAX_ITER, "%s: max_iter = %d outside [0, %d]", who, max_iter, GD_MAX_ITER);
  GPZ_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 15) == 0, "%s: partials must be 16-byte aligned", who);
  const GdPlan p = gd_plan(D, partials);
  GPZ_REQUIRE(partials_bytes >= p.bytes, "%s: partials too small (%zu bytes, %zu needed)", who, partials_bytes, p.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const GrRows r{row_ptr, row_spot, row_perm, col_val, N, D, nnz};
  GPZ_HIP_OK(hipMemsetAsync(info, 0, sizeof(int32_t), s));
  hipLaunchKernelGGL(gd_total_kernel, dim3(1), dim3(GR_THREADS), 0, s, size, N, p.totals, info);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(gd_kernel, dim3(unsigned(p.workgroups)), dim3(GR_THREADS), 0, s, r, size, p.totals, theta_min, theta_max,
                     int(max_iter), theta, gain, poisson_loglik, status, iterations, info);
  GPZ_LAUNCH_OK();
  return 0;
}
