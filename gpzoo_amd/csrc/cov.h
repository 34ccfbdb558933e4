// cov.h -- fp32 covariance of one (point, point) pair, shared by the stand-alone fill (kfill.hip) and by the
// stage-1 product that generates its Kzx operand itself (gemmw.hip, WB_GEN): one definition, explicit
// operation order, no contraction left to the compiler, so both paths produce the same bits.
//
// Replaces the element-wise part of kernels.py:14-30 (Matern-3/2, and the two closed forms a user of the reference most
// often puts in its place: Matern-1/2 and Matern-5/2) and :42-58 / :118-130 (RBF).  KIND is the ABI's kernel kind
// (GPZ_KERNEL_*): 0 RBF, 1 Matern-3/2, 4 Matern-1/2, 5 Matern-5/2.
#pragma once
#include <hip/hip_runtime.h>

namespace gpz {

// Per-latent constants: amp = sigma^2; RBF: c0 = -0.5 / ell^2 * log2(e); Matern-3/2: c0 = sigma^2 sqrt(3) / ell,
// c1 = sqrt(3) / ell * log2(e) (the exponent goes through v_exp_f32 = 2^x); Matern-1/2: c1 = 1 / ell * log2(e), c0 unused;
// Matern-5/2: c0 = sigma^2 sqrt(5) / ell, c2 = sigma^2 5 / (3 ell^2), c1 = sqrt(5) / ell * log2(e).  amp, c0 (Matern) and c2
// carry the amplitude: a caller that zeroes padding through the constants zeroes all three.
struct CovConst { float amp, c0, c1, c2; };

template <int KIND>
__device__ __forceinline__ CovConst cov_const(float sigma, float ell) {
#pragma clang fp contract(off)
  CovConst c;
  c.amp = sigma * sigma;
  c.c2 = 0.f;
  if (KIND == 4) {
    c.c0 = 0.f;
    c.c1 = (1.f / ell) * 1.44269504088896341f;
  } else if (KIND == 5) {
    const float a = 2.2360679774997896964f / ell;
    c.c0 = c.amp * a;
    c.c1 = a * 1.44269504088896341f;
    c.c2 = c.amp * ((a * a) * 0.333333333333333333f);
  } else if (KIND == 1) {
    const float a = 1.7320508075688772935f / ell;
    c.c0 = c.amp * a;
    c.c1 = a * 1.44269504088896341f;
  } else {
    c.c0 = (-0.5f / (ell * ell)) * 1.44269504088896341f;
    c.c1 = 0.f;
  }
  return c;
}

// Squared distance by direct differencing, coordinates in order (50x more accurate in fp32 than
// the matmul expansion of torch.cdist).
template <int D>
__device__ __forceinline__ float cov_d2(const float* a, const float* b) {
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < D; ++k) { const float df = a[k] - b[k]; acc = __builtin_fmaf(df, df, acc); }
  return acc;
}

// The part of the evaluation that does not depend on the latent: RBF keeps d^2, Matern takes r = sqrt(d^2)
// (v_sqrt_f32, 1 ulp: the correctly rounded sqrtf costs 15 instructions per element).
template <int KIND>
__device__ __forceinline__ float cov_radial(float d2) {
  return (KIND == 1 || KIND == 4 || KIND == 5) ? __builtin_amdgcn_sqrtf(d2) : d2;
}

template <int KIND>
__device__ __forceinline__ float cov_value(float s, float amp, float c0, float c1, float c2) {
#pragma clang fp contract(off)
  if (KIND == 4) return amp * __builtin_amdgcn_exp2f(-(c1 * s));  // sigma^2 exp(-r / ell)
  if (KIND == 5) {
    const float quad = __builtin_fmaf(__builtin_fmaf(c2, s, c0), s, amp);   // sigma^2 (1 + v + v^2 / 3), v = sqrt(5) r / ell
    return quad * __builtin_amdgcn_exp2f(-(c1 * s));                        // exp(-v)
  }
  if (KIND == 1) {
    const float lin = __builtin_fmaf(c0, s, amp);                // sigma^2 (1 + sqrt(3) r / ell)
    return lin * __builtin_amdgcn_exp2f(-(c1 * s));              // exp(-sqrt(3) r / ell)
  }
  return amp * __builtin_amdgcn_exp2f(c0 * s);                   // sigma^2 exp(-d^2 / (2 ell^2))
}

// fp64 covariance of UNIT amplitude of one (point, point) pair, for the per-gene projection (gene_gp.hip): the operations of
// gram.hip's GramCov<double, KIND> in its order, so that with sigma = 1 (amp = 1 multiplies exactly) both generate the same
// bits -- the collapsed bound of gene_gp.hip needs K_zx y and K_zx K_xz to come from one K_zx.  coef() is the per-latent
// constant, radial() the part that does not depend on the latent (d^2 for RBF, r = sqrt(d^2) for the Matern kinds; unused
// coordinates are 0 on both sides), unit() the covariance at it.  Every fused multiply-add is written out, so the bits do not
// depend on the contraction setting of the file that includes this.
template <int KIND> struct CovF64 {
  static __device__ __forceinline__ double coef(double e) {
    return (KIND == 1) ? 1.7320508075688772935 / e : (KIND == 4) ? 1.0 / e : (KIND == 5) ? 2.2360679774997896964 / e : -0.5 / (e * e);
  }
  static __device__ __forceinline__ double radial(const double* z, const double* x, bool low_d) {
    double acc = 0.0;
    const int nd = low_d ? 2 : 4;
    for (int k = 0; k < nd; ++k) { const double df = z[k] - x[k]; acc = fma(df, df, acc); }
    return KIND == 0 ? acc : sqrt(acc);
  }
  static __device__ __forceinline__ double unit(double cf, double rad) {
    if (KIND == 0) return exp(cf * rad);
    const double t = cf * rad;
    if (KIND == 4) return exp(-t);
    const double lin = fma(cf, rad, 1.0);          // gram.hip's 1.0 + t, which its -ffp-contract=fast fuses with t = cf * rad
    if (KIND == 1) return lin * exp(-t);
    return (lin + t * t / 3.0) * exp(-t);
  }
};

}  // namespace gpz
