// nb.hip -- Monte-Carlo expected negative-binomial log-likelihood of the NSF factor models and its gradients, fused
// like poisson.hip: the (E, D, N) rate never exists in HBM and the workspace holds nothing of D x N elements.
//
// torch's parameterisation (distributions.NegativeBinomial(total_count = theta, logits = log mu - log theta)): per gene an
// inverse dispersion theta[d] > 0, mean mu = V[n] Z[e,d,n] with Z = sum_l W[d,l] exp(F[e,l,n]), F = mean + scale eps,
// variance mu + mu^2 / theta.  With x = mu / theta:
//   ll[e,d,n]  = y log x - (y + theta) log1p(x)  +  [lgamma(y + theta) - lgamma(theta)]  -  lgamma(y + 1)
//   G          = (1/E) (y / Z - V (y + theta) / (mu + theta))              (= d ll / d Z)
//   dW[d,l]    = sum_{e,n} G expF,   dexpF[e,l,n] = sum_d G W[d,l],   dmean = sum_e dexpF expF,  dscale = sum_e dexpF expF eps
//   dV[n]      = (1/E) sum_{e,d} (y / V - Z (y + theta) / (mu + theta))
//   dtheta[d]  = sum_n [psi(y + theta) - psi(theta)]  +  (1/E) sum_{e,n} ( -log1p(x) - E G Z / theta )
// (y log x - (y + theta) log1p(x) is y log(mu / (mu + theta)) - theta log1p(mu / theta); (mu - y) / (mu + theta) is
// -E G Z / theta, so the pass that forms G has dtheta's sample-dependent term for one more log1p.)
// loglik[0] is everything but -sum lgamma(y + 1), loglik[1] = sum lgamma(y + 1) (0 without with_lgamma).
//
// log1p is COMPENSATED: u = 1 + x, log1p(x) = log(u) + (x - (u - 1)) / u.  The rounding of 1 + x is what the plain
// log(1 + x) loses; near the Poisson limit (theta = 1e4, x ~ 1e-4) that is 1e-3 of max |dtheta| in fp32, because dtheta's
// terms cancel to O(1 / theta^2) there.  The correction reuses the reciprocal of u that (y + theta) / (mu + theta) =
// (y + theta) / (theta u) needs anyway, so it costs a subtraction and two multiply-adds, no third reciprocal.
//
// Work split (fp32, the three dense products on v_mfma_f32_16x16x4_f32, fp64 block sums, no atomics -> bitwise reproducible):
//   nb_prep_kernel    expF (E,Lt,N) and 1 / theta (D) once
//   nb_spot_kernel    pass A: rate tiles with genes as rows -> log-lik, dV and dexpF = W^T G partial slabs
//   nb_const_kernel   the bracketed terms above, which depend on y and theta only: one workgroup per gene, fp64
//   nb_gene_kernel    pass B: the transposed tiles (spots as rows) -> dW = G expF^T and dtheta's sample-dependent sum
//   nb_finish_kernel  sums the slabs into dmean, dscale, dV, dW, dtheta and the scalar
// Both passes are the templates of nb_passes.h, which nb_sparse.hip's zero part shares; this file supplies the policy with
// the counts as an operand (NbDense).  Their layout -- which lane holds which element, how one product's accumulators are
// the next one's operand without a transpose through LDS, the double-buffered operands -- is poisson.hip's and is described
// there.  poisson.hip does not share them: its pass A runs two waves per SIMD at the 256-VGPR limit, and any textual change
// re-rolls its register allocation ("Why the Poisson passes keep their own text").
#include "common.h"
#include "mmops.h"
#include "nb_passes.h"

namespace gpz {
namespace nb {

constexpr int NMAXL = 64;   // factors (PMAXL of poisson.hip)
constexpr int NMAXE = 32;   // samples per call (PMAXE)

struct NbArgs {
  const float* mean; const float* scale; const float* eps;   // (Lt,N), (Lt,N), (E,Lt,N)
  const float* W; const float* V; const float* theta; const float* y;   // (D,Lt), (N,), (D,), (D,N)
  float* expF; float* ith;                                   // (E,Lt,N), (D,) = 1 / theta
  float* dexp_slab; float* dV_slab; double* ll_slab;          // [SD][E][Lt][N], [SV][N], [S][nblk * E]
  float* dW_slab; double* dth_slab;                           // [SN][D][Lt], [SN][D]
  double* cl; double* cpsi; double* lg;                       // (D,) each: sums over spots of the y / theta-only terms
  float* dW; float* dmean; float* dscale; float* dV; float* dtheta; double* loglik;
  int64_t N, D;
  int Lt, E, S, with_lgamma;
  int SD, SV, SN;
};

__global__ void nb_prep_kernel(NbArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t per = (int64_t)a.Lt * a.N;
  if (i < a.D) a.ith[i] = 1.f / a.theta[i];
  if (i >= per * a.E) return;
  const int64_t ln = i % per;
  a.expF[i] = __expf(a.mean[ln] + a.scale[ln] * a.eps[i]);
}

// The element-wise part of both passes.  In: the rate factor zz = Z, the count, V of the spot, theta and 1 / theta of the
// gene.  With mu = V Z, x = mu / theta, u = 1 + x and t = (y + theta) / (mu + theta) = (y / theta + 1) / u:
//   lu = log2(u), c = (x - (u - 1)) / u       log1p(x) = ln2 lu + c   (the compensation, see the head of the file)
//   w  = y - mu t                             = theta (y - mu) / (mu + theta): dV = sum w / V, dtheta's term is -w / theta
//   g  = w / Z                                = y / Z - V t = E G
// Four transcendentals per element in pass A (two reciprocals, log2 u and log2 x for the value), three in pass B.
// u and c's numerator are each formed in one rounding, fma(mu, 1 / theta, 1) and fma(mu, 1 / theta, -(u - 1)), everywhere but
// in pass A's interior tiles (FUSED = false), which use the rounded x in both.  The forms are written out because the
// results are held bit for bit and the compiler's own choice between them changes with the text around the element.
struct NbElem { float x, lu, c, w, g; };
template <bool FUSED>
__device__ __forceinline__ NbElem nb_elem(float zz, float y1, float v, float ith) {
  NbElem o;
  const float mu = v * zz;
  o.x = mu * ith;
  float u, num;
  if constexpr (FUSED) {
    u = __builtin_fmaf(mu, ith, 1.f);
    num = __builtin_fmaf(mu, ith, -(u - 1.f));
  } else {
    asm("" : "+v"(o.x));                        // the rounded product: keeps what follows from being fused with it
    u = 1.f + o.x;
    num = o.x - (u - 1.f);
  }
  const float ru = __builtin_amdgcn_rcpf(u);
  o.lu = __builtin_amdgcn_logf(u);
  o.c = num * ru;
  const float t = __builtin_fmaf(y1, ith, 1.f) * ru;
  o.w = __builtin_fmaf(-mu, t, y1);
  o.g = o.w * __builtin_amdgcn_rcpf(zz);
  return o;
}

// What nb_passes.h asks of a step: the counts are an operand.
struct NbDense {
  static constexpr bool HAS_Y = true;
  static __device__ __forceinline__ int64_t spots(const NbArgs& a) { return a.N; }
  static __device__ __forceinline__ const float* y(const NbArgs& a) { return a.y; }
  // pass A, value: ln2 (y log2 x - (y + theta) log2 u) - (y + theta) c, the two parts summed apart and combined per group
  struct SumsA { float lla = 0.f, llb = 0.f; };
  template <bool MASKED>
  static __device__ __forceinline__ float elem_a(SumsA& s, int, float z, float y1, float v, float th, float ith, float& dv, bool ok) {
    const float yt = y1 + th;
    if constexpr (!MASKED) {
      const NbElem o = nb_elem<false>(z, y1, v, ith);
      s.lla = __builtin_fmaf(y1, __builtin_amdgcn_logf(o.x), s.lla);
      s.lla = __builtin_fmaf(-yt, o.lu, s.lla);
      s.llb = __builtin_fmaf(yt, o.c, s.llb);
      dv += o.w;
      return o.g;
    } else {
      const float zz = ok ? z : 1.f;
      const NbElem o = nb_elem<true>(zz, y1, v, ith);
      s.lla += ok ? __builtin_fmaf(y1, __builtin_amdgcn_logf(o.x), -yt * o.lu) : 0.f;
      s.llb += ok ? yt * o.c : 0.f;
      dv += ok ? o.w : 0.f;
      return ok ? o.g : 0.f;
    }
  }
  static __device__ __forceinline__ double fold_a(const SumsA& s, const float (&)[4]) { return (double)__builtin_fmaf(LN2, s.lla, -s.llb); }
  // dv holds sum_d w = V sum_d (y / V - Z t)
  static __device__ __forceinline__ float close_dv(float dv, float v, float inv_e) { return dv * __builtin_amdgcn_rcpf(v) * inv_e; }
  // pass B, dtheta's term: -log1p(x) - w / theta = -(ln2 lu + c) - w / theta, the three sums apart and combined per tile
  struct SumsB { float tpa = 0.f, tpb = 0.f, tpc = 0.f; };
  template <bool MASKED>
  static __device__ __forceinline__ float elem_b(SumsB& s, float z, float y1, float v, float ith, bool ok) {
    if constexpr (!MASKED) {
      const NbElem o = nb_elem<true>(z, y1, v, ith);
      s.tpa += o.lu;
      s.tpb += o.c;
      s.tpc += o.w;
      return o.g;
    } else {
      const float zz = ok ? z : 1.f, v1 = ok ? v : 1.f;
      const NbElem o = nb_elem<true>(zz, y1, v1, ith);
      s.tpa += ok ? o.lu : 0.f;
      s.tpb += ok ? o.c : 0.f;
      s.tpc += ok ? o.w : 0.f;
      return ok ? o.g : 0.f;
    }
  }
  static __device__ __forceinline__ double fold_b(const SumsB& s, float ith) { return -(double)(__builtin_fmaf(LN2, s.tpa, s.tpb) + ith * s.tpc); }
};

// Pass A  grid (E * ceil(N/64), S), 4 waves: nb_pass_a of nb_passes.h.
#ifndef GPZ_NB_SPOT_WAVES
#define GPZ_NB_SPOT_WAVES 1     // waves per SIMD the register allocation of pass A is made for
#endif
template <int KS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(GPZ_NB_SPOT_WAVES, GPZ_NB_SPOT_WAVES))) void nb_spot_kernel(NbArgs a, int GS) {
  nb_pass_a<KS, NbDense>(a, GS);
}

// The terms that depend on y and theta only: per gene, sums over its spots of lgamma(y + theta) - lgamma(theta) (-> cl),
// psi(y + theta) - psi(theta) (-> cpsi) and lgamma(y + 1) (-> lg).  They vanish at y = 0 and do not depend on the sample,
// so they have their own pass over y -- one workgroup per gene, fp64, a fixed order -- instead of a branch per element in
// the MFMA loops.  Integer 0 < y < 16: the recurrences.  With p_k = prod_{j<k} (theta + j) and q_k = q_{k-1} (theta + k-1) +
// p_{k-1}, sum_{k<y} 1 / (theta + k) = q_y / p_y (one division per element) and sum_{k<y} log(theta + k) = log p_y; the p_y
// of a thread's elements are multiplied up and the logarithm is taken when the running product leaves [1e-150, 1e150]
// (p_y <= 1e120 for theta < 1e8), so an fp64 log is paid once per dozens of counts.  Every other count (16 and above, or
// not an integer) needs lgamma and digamma_pos, hundreds of fp64 instructions that a whole wave would wait for whenever
// one of its 64 counts is such a one -- at theta = 0.3 that is most waves.  Those counts are set aside instead: each wave
// appends them to a list of its own in LDS (positions from a ballot: the order is fixed) and works the list off with all
// lanes busy, when it is full and at the end; lgamma(theta) and psi(theta) enter as one more entry of weight -count.
// A thread has NB_UNROLL loads of y in flight per step: with one, the pass waited out the memory latency 1 900 times per
// SIMD at Slide-seq size (1.0 ms for 0.5 GB).
constexpr int NB_LIST = 1024;                   // set-aside counts per wave
constexpr int NB_UNROLL = 8;                    // counts per thread and step
__global__ __launch_bounds__(256) void nb_const_kernel(NbArgs a) {
  __shared__ double sh[8];
  __shared__ float lfact[256];
  __shared__ float slow[4][NB_LIST];
  for (int i = threadIdx.x; i < 256; i += 256) lfact[i] = lgammaf((float)i + 1.f);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t d = blockIdx.x;
  const double th = (double)a.theta[d];
  const bool rec = th > 1e-20 && th < 1e8;
  const float* yr = a.y + d * a.N;
  float* lst = slow[wave];
  double cl = 0.0, cp = 0.0, lg = 0.0, run = 1.0;
  int cnt = 0;                                  // entries of this wave's list (the same in all its lanes)
  for (int64_t base = 0;; base += 256 * NB_UNROLL) {
    const bool more = base < a.N;               // (uniform over the workgroup)
    if (more) {
      float yy[NB_UNROLL];
#pragma unroll
      for (int j = 0; j < NB_UNROLL; ++j) {
        const int64_t n = base + 256 * j + threadIdx.x;
        yy[j] = n < a.N ? yr[n] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < NB_UNROLL; ++j) {
      const float y1 = yy[j];
      const int yi = (int)y1;
      const bool whole = y1 == (float)yi && yi > 0;
      const bool fast = whole && yi < 16 && rec;
      if (fast) {
        double p = th, q = 1.0;
        for (int k = 1; k < yi; ++k) { const double f = th + k; q = __builtin_fma(q, f, p); p *= f; }
        cp += q / p;
        run *= p;
        if (run > 1e150 || run < 1e-150) { cl += log(run); run = 1.0; }
      }
      const bool aside = y1 != 0.f && !fast;
      const unsigned long long m = __ballot(aside);
      if (aside) lst[cnt + __popcll(m & ((1ull << lane) - 1ull))] = y1;
      cnt += __popcll(m);
      if (a.with_lgamma && y1 != 0.f) lg += (double)lgamma1p_term(lfact, y1, yi, whole);
      }
    }
    __syncthreads();
    if (cnt > NB_LIST - 64 * NB_UNROLL || (!more && cnt > 0)) {
      for (int j = lane; j <= cnt; j += 64) {
        const bool last = j == cnt;             // lgamma(theta), psi(theta), once for all the entries
        const double yt = (last ? 0.0 : (double)lst[j]) + th;
        const double wgt = last ? -(double)cnt : 1.0;
        cl += wgt * lgamma(yt);
        cp += wgt * digamma_pos(yt);
      }
      cnt = 0;
    }
    __syncthreads();
    if (!more) break;
  }
  cl += log(run);
  const double tcl = block_sum(cl, sh);
  const double tcp = block_sum(cp, sh);
  const double tlg = block_sum(lg, sh);
  if (threadIdx.x == 0) { a.cl[d] = tcl; a.cpsi[d] = tcp; a.lg[d] = tlg; }
}

// Pass B  grid (ceil(D/64), SN), 4 waves: nb_pass_b of nb_passes.h.
template <int KS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 4))) void nb_gene_kernel(NbArgs a, int SN) {
  nb_pass_b<KS, NbDense>(a, SN);
}

// dmean, dscale (Lt,N), dV (N), dW (D,Lt) and dtheta (D) from the slabs (fixed summation order); log-lik total
__global__ __launch_bounds__(256) void nb_finish_kernel(NbArgs a, int nblk_spot) {
  __shared__ double sh[8];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t per = (int64_t)a.Lt * a.N;
  if (i < per) {
    float dm = 0.f, ds = 0.f;
    for (int e = 0; e < a.E; ++e) {
      float dx = 0.f;
      for (int s = 0; s < a.SD; ++s) dx += a.dexp_slab[((int64_t)s * a.E + e) * per + i];
      const float dF = dx * a.expF[e * per + i];
      dm += dF;
      ds += dF * a.eps[e * per + i];
    }
    a.dmean[i] = dm;
    a.dscale[i] = ds;
  }
  if (i < a.N) {
    float dv = 0.f;
    for (int s = 0; s < a.SV; ++s) dv += a.dV_slab[(int64_t)s * a.N + i];
    a.dV[i] = dv;
  }
  const int64_t dl = a.D * a.Lt;
  for (int64_t j = i; j < dl; j += (int64_t)gridDim.x * 256) {
    float w = 0.f;
    for (int s = 0; s < a.SN; ++s) w += a.dW_slab[(int64_t)s * dl + j];
    a.dW[j] = w;
  }
  for (int64_t j = i; j < a.D; j += (int64_t)gridDim.x * 256) {
    double t = a.cpsi[j];
    for (int s = 0; s < a.SN; ++s) t += a.dth_slab[(int64_t)s * a.D + j];
    a.dtheta[j] = (float)t;
  }
  if (blockIdx.x == 0) {
    double v = 0.0, vc = 0.0, vg = 0.0;
    for (int j = threadIdx.x; j < a.S * nblk_spot; j += 256) v += a.ll_slab[j];
    for (int64_t j = threadIdx.x; j < a.D; j += 256) { vc += a.cl[j]; vg += a.lg[j]; }
    const double t = block_sum(v, sh);
    const double tc = block_sum(vc, sh);
    const double tg = block_sum(vg, sh);
    if (threadIdx.x == 0) { a.loglik[0] = t + tc; a.loglik[1] = tg; }
  }
}

// k-steps of 4 factors of the kernel instance that serves Lt factors.  Nine instances: 1 .. 4, 5 .. 8, 9 .. 16, 17 .. 20 (the
// notebooks' NSF models run 20), 21 .. 24, 25 .. 32, 33 .. 40 (their hybrids run 39 .. 40), 41 .. 48 and 49 .. 64 factors.
static int nb_ksteps(int Lt) {
  const int k = (Lt + 3) / 4;
  if (k <= 2) return k;
  if (k <= 4) return 4;
  if (k <= 6) return k;
  if (k <= 8) return 8;
  if (k <= 10) return 10;
  if (k <= 12) return 12;
  return 16;
}

struct NbPlan { int S, GS, SN; int64_t nblk; size_t bytes; float *expF, *ith, *dexp, *dVs, *dWs; double *ll, *dth, *cl, *cpsi, *lg; };

static NbPlan nb_plan(int64_t N, int64_t D, int Lt, int E, void* ws) {
  NbPlan pl;
  const SlicePlan sp = slice_plan(N, D, E);
  pl.S = sp.S; pl.GS = sp.GS; pl.SN = sp.SN; pl.nblk = sp.nblk;
  Carver c(ws);
  pl.expF = c.take<float>((int64_t)E * Lt * N);
  pl.ith = c.take<float>(D);
  pl.dexp = c.take<float>((int64_t)pl.S * pl.GS * E * Lt * N);
  pl.dVs = c.take<float>((int64_t)pl.S * E * pl.GS * N);
  pl.dWs = c.take<float>((int64_t)pl.SN * D * Lt);
  pl.ll = c.take<double>((int64_t)pl.S * pl.nblk * E);
  pl.dth = c.take<double>((int64_t)pl.SN * D);
  pl.cl = c.take<double>(D);
  pl.cpsi = c.take<double>(D);
  pl.lg = c.take<double>(D);
  pl.bytes = c.used();
  return pl;
}

static bool nb_extents_ok(int64_t N, int64_t D, int Lt, int E) {
  if (N < 1 || D < 1) { set_error("gpz_nb_nsf: bad extents"); return false; }
  if (D >= (1ll << 31)) { set_error("gpz_nb_nsf: D = %lld genes exceed the 2^31 - 1 a call can address", (long long)D); return false; }
  if (Lt < 1 || Lt > NMAXL) { set_error("gpz_nb_nsf: %d factors unsupported (1..%d)", Lt, NMAXL); return false; }
  if (E < 1 || E > NMAXE) { set_error("gpz_nb_nsf: %d samples per call unsupported (1..%d)", E, NMAXE); return false; }
  // nb_gene_kernel addresses exp(F) through a buffer descriptor with 32-bit byte extents and offsets
  if ((int64_t)E * Lt * N * 4 >= (1ll << 31)) {
    set_error("gpz_nb_nsf: E * Lt * N = %lld elements of exp(F) exceed the 2 GiB a call can address: split N",
              (long long)((int64_t)E * Lt * N));
    return false;
  }
  return true;
}

template <int KS>
static int nb_passes(const NbArgs& a, const NbPlan& pl, hipStream_t s) {
  const size_t lds = pass_b_lds(KS, a.E < PASS_EG ? a.E : PASS_EG);
  static_assert(pass_b_lds(KS, PASS_EG) <= 160 * 1024, "nb_gene_kernel: LDS of the largest sample group");
  if (int rc = lds_opt_in<nb_gene_kernel<KS>>(pass_b_lds(KS, PASS_EG))) return rc;
  hipLaunchKernelGGL((nb_spot_kernel<KS>), dim3((unsigned)(pl.nblk * a.E), (unsigned)pl.S), dim3(64 * pl.GS), 0, s, a, pl.GS);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(nb_const_kernel, dim3((unsigned)a.D), dim3(256), 0, s, a);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL((nb_gene_kernel<KS>), dim3((unsigned)((a.D + 63) / 64), (unsigned)pl.SN), dim3(256), lds, s, a, pl.SN);
  GPZ_LAUNCH_OK();
  return 0;
}

}  // namespace nb
}  // namespace gpz

using namespace gpz;
using namespace gpz::nb;

extern "C" int gpz_nb_nsf_plan(int64_t N, int64_t D, int32_t Lt, int32_t E, int32_t* factors_padded, int32_t* aligned_rows,
                               int32_t* gene_slices, int32_t* spot_slices) {
  if (!nb_extents_ok(N, D, Lt, E)) return -1;
  const NbPlan pl = nb_plan(N, D, Lt, E, nullptr);
  if (factors_padded) *factors_padded = 4 * nb_ksteps(Lt);
  if (aligned_rows) *aligned_rows = (N & 3) == 0;
  if (gene_slices) *gene_slices = pl.S;
  if (spot_slices) *spot_slices = pl.SN;
  return 0;
}

extern "C" size_t gpz_nb_nsf_workspace_bytes(int64_t N, int64_t D, int32_t Lt, int32_t E) {
  if (!nb_extents_ok(N, D, Lt, E)) return 0;
  return nb_plan(N, D, Lt, E, nullptr).bytes;
}

extern "C" int gpz_nb_nsf(const float* mean, const float* scale, const float* eps, const float* W, const float* V,
                          const float* theta, const float* y, int64_t N, int64_t D, int32_t Lt, int32_t E,
                          int32_t with_lgamma, double* loglik, float* dmean, float* dscale, float* dW, float* dV,
                          float* dtheta, void* ws, size_t ws_bytes, void* stream) {
  GPZ_REQUIRE(mean && scale && eps && W && V && theta && y && loglik && dmean && dscale && dW && dV && dtheta && ws,
              "gpz_nb_nsf: null pointer");
  {
    const void* arrays[] = {mean, scale, eps, W, V, theta, y, loglik, dmean, dscale, dW, dV, dtheta, ws};
    uintptr_t low = 0;
    for (const void* p : arrays) low |= reinterpret_cast<uintptr_t>(p);
    GPZ_REQUIRE((low & 15) == 0, "gpz_nb_nsf: every array argument and the workspace must be 16-byte aligned");
  }
  if (!nb_extents_ok(N, D, Lt, E)) return -1;
  NbPlan pl = nb_plan(N, D, Lt, E, ws);
  GPZ_REQUIRE(ws_bytes >= pl.bytes, "gpz_nb_nsf: workspace too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  NbArgs a;
  a.mean = mean; a.scale = scale; a.eps = eps; a.W = W; a.V = V; a.theta = theta; a.y = y;
  a.expF = pl.expF; a.ith = pl.ith; a.dexp_slab = pl.dexp; a.dV_slab = pl.dVs; a.ll_slab = pl.ll; a.dW_slab = pl.dWs;
  a.dth_slab = pl.dth; a.cl = pl.cl; a.cpsi = pl.cpsi; a.lg = pl.lg;
  a.dW = dW; a.dmean = dmean; a.dscale = dscale; a.dV = dV; a.dtheta = dtheta; a.loglik = loglik;
  a.N = N; a.D = D; a.Lt = Lt; a.E = E; a.S = pl.S; a.with_lgamma = with_lgamma;
  a.SD = pl.S * pl.GS; a.SV = pl.S * E * pl.GS; a.SN = pl.SN;
  int64_t tot = (int64_t)E * Lt * N;
  if (tot < D) tot = D;
  hipLaunchKernelGGL(nb_prep_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, a);
  GPZ_LAUNCH_OK();
  int rc;
  switch (nb_ksteps(Lt)) {
    case 1: rc = nb_passes<1>(a, pl, s); break;
    case 2: rc = nb_passes<2>(a, pl, s); break;
    case 4: rc = nb_passes<4>(a, pl, s); break;
    case 5: rc = nb_passes<5>(a, pl, s); break;
    case 6: rc = nb_passes<6>(a, pl, s); break;
    case 8: rc = nb_passes<8>(a, pl, s); break;
    case 10: rc = nb_passes<10>(a, pl, s); break;
    case 12: rc = nb_passes<12>(a, pl, s); break;
    default: rc = nb_passes<16>(a, pl, s); break;
  }
  if (rc) return rc;
  const int64_t per = (int64_t)Lt * N;
  hipLaunchKernelGGL(nb_finish_kernel, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, s, a, (int)(pl.nblk * E));
  GPZ_LAUNCH_OK();
  return 0;
}
