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
// The layout of both passes -- which lane holds which element, how one product's accumulators are the next one's operand
// without a transpose through LDS, the double-buffered operands -- is poisson.hip's and is described there; this file
// repeats the kernels with theta as a second per-gene operand because the Poisson object code must not change.
#include "common.h"
#include "mmops.h"

namespace gpz {
namespace nb {

constexpr int NMAXL = 64;   // factors (PMAXL of poisson.hip)
constexpr int NMAXE = 32;   // samples per call (PMAXE)
constexpr int NEG = 4;      // samples pass B holds in LDS at a time (PEG)
constexpr float LN2 = 0.69314718055994530942f;

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

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x2 pkfma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }

// The element-wise part of both passes.  In: the rate factor zz = Z, the count, V of the spot, theta and 1 / theta of the
// gene.  With mu = V Z, x = mu / theta, u = 1 + x and t = (y + theta) / (mu + theta) = (y / theta + 1) / u:
//   lu = log2(u), c = (x - (u - 1)) / u       log1p(x) = ln2 lu + c   (the compensation, see the head of the file)
//   w  = y - mu t                             = theta (y - mu) / (mu + theta): dV = sum w / V, dtheta's term is -w / theta
//   g  = w / Z                                = y / Z - V t = E G
// Four transcendentals per element in pass A (two reciprocals, log2 u and log2 x for the value), three in pass B.
struct NbElem { float x, lu, c, w, g; };
__device__ __forceinline__ NbElem nb_elem(float zz, float y1, float v, float ith) {
  NbElem o;
  const float mu = v * zz;
  o.x = mu * ith;
  const float u = 1.f + o.x;
  const float ru = __builtin_amdgcn_rcpf(u);
  o.lu = __builtin_amdgcn_logf(u);
  o.c = (o.x - (u - 1.f)) * ru;
  const float t = __builtin_fmaf(y1, ith, 1.f) * ru;
  o.w = __builtin_fmaf(-mu, t, y1);
  o.g = o.w * __builtin_amdgcn_rcpf(zz);
  return o;
}

// Pass A  grid (E * ceil(N/64), S), 4 waves; see spot_mfma_kernel of poisson.hip.
#ifndef GPZ_NB_SPOT_WAVES
#define GPZ_NB_SPOT_WAVES 1     // waves per SIMD the register allocation of pass A is made for
#endif
template <int KS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(GPZ_NB_SPOT_WAVES, GPZ_NB_SPOT_WAVES))) void nb_spot_kernel(NbArgs a, int GS) {
  constexpr int LT16 = (KS + 3) / 4;
  __shared__ double sh[8];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int e = blockIdx.x % a.E, gs = wave;
  const int s = blockIdx.y;
  const int64_t n0 = (int64_t)(blockIdx.x / a.E) * 64;
  const int64_t per = (int64_t)a.Lt * a.N;
  const int64_t dper = (a.D + a.S - 1) / a.S;
  const int64_t d_lo = s * dper, d_hi = (d_lo + dper < a.D) ? d_lo + dper : a.D;
  const float inv_e = 1.f / (float)a.E;
  const bool vec = (a.N & 3) == 0;
  const bool tile_full = n0 + 64 <= a.N;
  float vn[4], invv[4], bz[KS][4];
  bool nok[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int64_t n = n0 + 4 * r + c;
    nok[c] = n < a.N;
    vn[c] = nok[c] ? a.V[n] : 1.f;
    invv[c] = __builtin_amdgcn_rcpf(vn[c]);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int l = 4 * ks + q;
      bz[ks][c] = (nok[c] && l < a.Lt) ? a.expF[e * per + (int64_t)l * a.N + n] : 0.f;
    }
  }
  f32x4 dacc[LT16][4];
#pragma unroll
  for (int lt = 0; lt < LT16; ++lt)
#pragma unroll
    for (int c = 0; c < 4; ++c) dacc[lt][c] = f32x4{0, 0, 0, 0};
  float dv[4] = {0.f, 0.f, 0.f, 0.f};
  double ll = 0.0;
  // one 16-gene group's operands; th / ith are theta and 1 / theta of the genes 4q + g on this lane's register axis
  // (1 for a gene that does not exist: its elements are masked, but the arithmetic must stay finite)
  struct Group { float wa[KS]; f32x4 yv[4]; float wt[4][LT16]; float th[4], ith[4]; };
  auto load_group = [&](int64_t d0, Group& G) __attribute__((always_inline)) {
    if (d0 + 16 <= d_hi && tile_full && vec) {
      const float* wr = a.W + (d0 + r) * a.Lt;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int l = 4 * ks + q;
        const float v = wr[l < a.Lt ? l : a.Lt - 1];
        G.wa[ks] = l < a.Lt ? v : 0.f;
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int64_t dg = d0 + 4 * q + g;
        G.yv[g] = *reinterpret_cast<const f32x4*>(a.y + dg * a.N + n0 + 4 * r);
        G.th[g] = a.theta[dg];
        G.ith[g] = a.ith[dg];
        const float* wg = a.W + dg * a.Lt;
#pragma unroll
        for (int lt = 0; lt < LT16; ++lt) {
          const int l = 16 * lt + r;
          const float v = wg[l < a.Lt ? l : a.Lt - 1];
          G.wt[g][lt] = l < a.Lt ? v : 0.f;
        }
      }
      return;
    }
    const int64_t d = d0 + r;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int l = 4 * ks + q;
      G.wa[ks] = (d < d_hi && l < a.Lt) ? a.W[d * a.Lt + l] : 0.f;
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int64_t dg = d0 + 4 * q + g;
      G.yv[g] = f32x4{0, 0, 0, 0};
      G.th[g] = 1.f;
      G.ith[g] = 1.f;
      if (dg < d_hi) {
        G.th[g] = a.theta[dg];
        G.ith[g] = a.ith[dg];
        const float* yp = a.y + dg * a.N + n0 + 4 * r;
        if (vec && nok[3]) G.yv[g] = *reinterpret_cast<const f32x4*>(yp);
        else {
#pragma unroll
          for (int c = 0; c < 4; ++c) if (nok[c]) G.yv[g][c] = yp[c];
        }
      }
#pragma unroll
      for (int lt = 0; lt < LT16; ++lt) {
        const int l = 16 * lt + r;
        G.wt[g][lt] = (dg < d_hi && l < a.Lt) ? a.W[dg * a.Lt + l] : 0.f;
      }
    }
  };
  Group cur, nxt;
  const int64_t dstep = 16 * GS;
  int64_t d0 = d_lo + 16 * gs;
  if (d0 < d_hi) load_group(d0, cur);
  for (; d0 < d_hi; d0 += dstep) {
    if (d0 + dstep < d_hi) load_group(d0 + dstep, nxt);
    f32x4 z[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      z[c] = f32x4{0, 0, 0, 0};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) z[c] = mfma4(cur.wa[ks], bz[ks][c], z[c]);
    }
    // element-wise: the sample-dependent terms of the log-density, dV, and G in place of Z (1 / E applied at the end)
    // value: ln2 (y log2 x - (y + theta) log2 u) - (y + theta) c, the two parts summed apart and combined per group
    float lla = 0.f, llb = 0.f;
    if (d0 + 16 <= d_hi && tile_full) {
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float y1 = cur.yv[g][c], yt = y1 + cur.th[g];
          const NbElem o = nb_elem(z[c][g], y1, vn[c], cur.ith[g]);
          lla = __builtin_fmaf(y1, __builtin_amdgcn_logf(o.x), lla);
          lla = __builtin_fmaf(-yt, o.lu, lla);
          llb = __builtin_fmaf(yt, o.c, llb);
          dv[c] += o.w;
          z[c][g] = o.g;
        }
    } else {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const bool dok = d0 + 4 * q + g < d_hi;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const bool ok = dok && nok[c];
          const float zz = ok ? z[c][g] : 1.f, y1 = cur.yv[g][c], yt = y1 + cur.th[g];
          const NbElem o = nb_elem(zz, y1, vn[c], cur.ith[g]);
          lla += ok ? __builtin_fmaf(y1, __builtin_amdgcn_logf(o.x), -yt * o.lu) : 0.f;
          llb += ok ? yt * o.c : 0.f;
          dv[c] += ok ? o.w : 0.f;
          z[c][g] = ok ? o.g : 0.f;
        }
      }
    }
    ll += (double)__builtin_fmaf(LN2, lla, -llb);
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int lt = 0; lt < LT16; ++lt)
#pragma unroll
        for (int c = 0; c < 4; ++c) dacc[lt][c] = mfma4(cur.wt[g][lt], z[c][g], dacc[lt][c]);
    cur = nxt;
  }
  const int64_t slab = (int64_t)s * GS + gs;
#pragma unroll
  for (int lt = 0; lt < LT16; ++lt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int l = 16 * lt + 4 * q + g;
      if (l < a.Lt) {
        float* dp = a.dexp_slab + ((slab * a.E + e) * a.Lt + l) * a.N + n0 + 4 * r;
        if (vec && nok[3])
          *reinterpret_cast<f32x4*>(dp) = f32x4{dacc[lt][0][g] * inv_e, dacc[lt][1][g] * inv_e, dacc[lt][2][g] * inv_e, dacc[lt][3][g] * inv_e};
        else {
#pragma unroll
          for (int c = 0; c < 4; ++c) if (nok[c]) dp[c] = dacc[lt][c][g] * inv_e;
        }
      }
    }
  const int nw = a.E * GS;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    float v = dv[c] * invv[c] * inv_e;           // dv holds sum_d w = V sum_d (y / V - Z t)
    v += __shfl_xor(v, 16); v += __shfl_xor(v, 32);
    if (q == 0 && nok[c]) a.dV_slab[((int64_t)s * nw + e * GS + gs) * a.N + n0 + 4 * r + c] = v;
  }
  const double t = block_sum(ll * (double)inv_e, sh);
  if (threadIdx.x == 0) a.ll_slab[(int64_t)s * gridDim.x + blockIdx.x] = t;
}

// psi(x), x > 0, fp64: the argument shifted above 6 by psi(x) = psi(x + 1) - 1 / x, then the asymptotic series (its first
// omitted term is below 1e-12 there)
__device__ __forceinline__ double digamma_pos(double x) {
  double r = 0.0;
  while (x < 6.0) { r -= 1.0 / x; x += 1.0; }
  const double i = 1.0 / x, i2 = i * i;
  const double ser = i2 * (1.0 / 12 - i2 * (1.0 / 120 - i2 * (1.0 / 252 - i2 * (1.0 / 240 - i2 * (1.0 / 132 - i2 * (691.0 / 32760 - i2 / 12))))));
  return r + log(x) - 0.5 * i - ser;
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
      if (a.with_lgamma && y1 != 0.f) lg += (double)((whole && yi < 256) ? lfact[yi] : lgammaf(y1 + 1.f));
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

// Pass B  grid (ceil(D/64), SN), 4 waves; see gene_mfma_kernel of poisson.hip.  This lane's gene is column r of the
// transposed tile, so theta is one register, and dtheta's sample-dependent sum reduces over the same axes as dW: one more
// output column per gene.
template <int KS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 4))) void nb_gene_kernel(NbArgs a, int SN) {
  constexpr bool TAIL = (KS % 4) == 1;
  constexpr int LTM = TAIL ? KS / 4 : (KS + 3) / 4, LTA = LTM > 0 ? LTM : 1, L0 = 16 * LTM;
  constexpr int LT16 = (KS + 3) / 4, LP = 16 * LT16, PF = 68;
  extern __shared__ float smem_nb[];
  const int EG = a.E < NEG ? a.E : NEG, NG = (a.E + EG - 1) / EG;
  const int FB = EG * LP * PF;
  float* sF = smem_nb;                          // [2][EG][LP][PF]
  float* sV = smem_nb + 2 * FB;                 // [2][64]
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int64_t d0 = ((int64_t)blockIdx.x * 4 + wave) * 16;
  const int64_t dcol = d0 + r;
  const bool dok = dcol < a.D;
  const bool d_full = d0 + 16 <= a.D;
  const int64_t per = (int64_t)a.Lt * a.N;
  const int64_t ntiles = (a.N + 63) / 64, tper = (ntiles + SN - 1) / SN;
  const int64_t t_lo = blockIdx.y * tper, t_hi = (t_lo + tper < ntiles) ? t_lo + tper : ntiles;
  const float inv_e = 1.f / (float)a.E;
  const bool vec = (a.N & 3) == 0;
  const float ith = dok ? a.ith[dcol] : 1.f;
  float wb[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int l = 4 * ks + q;
    wb[ks] = (dok && l < a.Lt) ? a.W[dcol * a.Lt + l] : 0.f;
  }
  f32x4 dwt[LTA];
#pragma unroll
  for (int lt = 0; lt < LTA; ++lt) dwt[lt] = f32x4{0, 0, 0, 0};
  f32x2 tw[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) tw[t] = f32x2{0.f, 0.f};
  double dth = 0.0;                             // sum over this lane's spots and all samples of -log1p(x) - E G Z / theta
  const int arow = 16 * (r >> 2) + (r & 3);
  typedef __attribute__((address_space(3))) void lds_void;
  for (int i = threadIdx.x; i < 2 * FB; i += 256) sF[i] = 0.f;
  __syncthreads();
#if defined(__HIP_DEVICE_COMPILE__)
  const __amdgpu_buffer_rsrc_t f_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.expF), 0, (int)((int64_t)a.E * per * sizeof(float)), 0x00020000);
  const __amdgpu_buffer_rsrc_t v_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.V), 0, (int)(a.N * sizeof(float)), 0x00020000);
#endif
  auto stage = [&](int64_t tt, int gi, int buf) __attribute__((always_inline)) {
#if defined(__HIP_DEVICE_COMPILE__)
    const int64_t n0 = tt * 64;
    const int e0 = gi * EG, ne = (a.E - e0 < EG) ? a.E - e0 : EG;
    for (int el = 0; el < ne; ++el)
      for (int l = wave; l < a.Lt; l += 4)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(f_rsrc, (lds_void*)(sF + buf * FB + (el * LP + l) * PF), 4, lane * 4,
                                                 (int)(((e0 + el) * per + (int64_t)l * a.N + n0) * 4), 0, 0);
    if (wave == 0)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(v_rsrc, (lds_void*)(sV + buf * 64), 4, lane * 4, (int)(n0 * 4), 0, 0);
#endif
  };
  auto load_y = [&](int64_t tt, f32x4 (&yv)[4]) __attribute__((always_inline)) {
    const int64_t n0 = tt * 64;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int64_t n = n0 + 16 * q + 4 * c;
      yv[c] = f32x4{0, 0, 0, 0};
      if (dok) {
        const float* yp = a.y + dcol * a.N + n;
        if (vec && n + 3 < a.N) yv[c] = *reinterpret_cast<const f32x4*>(yp);
        else {
#pragma unroll
          for (int g = 0; g < 4; ++g) if (n + g < a.N) yv[c][g] = yp[g];
        }
      }
    }
  };
  f32x4 yv[4], yn[4];
  if (t_lo < t_hi) { stage(t_lo, 0, 0); load_y(t_lo, yv); }
  int buf = 0;
  for (int64_t tt = t_lo; tt < t_hi; ++tt) {
    const int64_t n0 = tt * 64;
    for (int gi = 0; gi < NG; ++gi, buf ^= 1) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (gi + 1 < NG) stage(tt, gi + 1, buf ^ 1);
      else if (tt + 1 < t_hi) { stage(tt + 1, 0, buf ^ 1); load_y(tt + 1, yn); }
      f32x4 vv[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) vv[c] = *reinterpret_cast<const f32x4*>(sV + buf * 64 + 16 * q + 4 * c);
      const int ne = (a.E - gi * EG < EG) ? a.E - gi * EG : EG;
      for (int e = 0; e < ne; ++e) {
        const float* fe = sF + buf * FB + e * LP * PF;
        f32x4 z[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          z[c] = f32x4{0, 0, 0, 0};
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) z[c] = mfma4(fe[(4 * ks + q) * PF + arow + 4 * c], wb[ks], z[c]);
        }
        // G^T in place of Z^T (1 / E applied at the end) and dtheta's term; a spot past N reads V = 0 or a finite
        // neighbour through the buffer descriptor, so the masked form replaces V as well as Z
        // (dtheta's term is -log1p(x) - w / theta = -(ln2 lu + c) - w / theta: the three sums apart, combined per tile)
        float tpa = 0.f, tpb = 0.f, tpc = 0.f;
        if (d_full && n0 + 64 <= a.N) {
#pragma unroll
          for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              const NbElem o = nb_elem(z[c][g], yv[c][g], vv[c][g], ith);
              tpa += o.lu;
              tpb += o.c;
              tpc += o.w;
              z[c][g] = o.g;
            }
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              const bool ok = dok && n0 + 16 * q + 4 * c + g < a.N;
              const float zz = ok ? z[c][g] : 1.f, v1 = ok ? vv[c][g] : 1.f;
              const NbElem o = nb_elem(zz, yv[c][g], v1, ith);
              tpa += ok ? o.lu : 0.f;
              tpb += ok ? o.c : 0.f;
              tpc += ok ? o.w : 0.f;
              z[c][g] = ok ? o.g : 0.f;
            }
        }
        dth -= (double)(__builtin_fmaf(LN2, tpa, tpb) + ith * tpc);   // fp32 sums of 16 terms, fp64 across tiles and samples
#pragma unroll
        for (int lt = 0; lt < LTM; ++lt)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const f32x4 fa = *reinterpret_cast<const f32x4*>(fe + (16 * lt + r) * PF + 16 * q + 4 * c);
#pragma unroll
            for (int g = 0; g < 4; ++g) dwt[lt] = mfma4(fa[g], z[c][g], dwt[lt]);
          }
        if constexpr (TAIL) {
#pragma unroll
          for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const f32x4 fv = *reinterpret_cast<const f32x4*>(fe + (L0 + t) * PF + 16 * q + 4 * c);
              tw[t] = pkfma(f32x2{z[c][0], z[c][1]}, f32x2{fv[0], fv[1]}, tw[t]);
              tw[t] = pkfma(f32x2{z[c][2], z[c][3]}, f32x2{fv[2], fv[3]}, tw[t]);
            }
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) yv[c] = yn[c];
  }
  if constexpr (TAIL) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      float v = (tw[t][0] + tw[t][1]) * inv_e;
      v += __shfl_xor(v, 16); v += __shfl_xor(v, 32);
      if (q == 0 && dok && L0 + t < a.Lt) a.dW_slab[((int64_t)blockIdx.y * a.D + dcol) * a.Lt + L0 + t] = v;
    }
  }
  {
    double v = dth * (double)inv_e;
    v += __shfl_xor(v, 16); v += __shfl_xor(v, 32);
    if (q == 0 && dok) a.dth_slab[(int64_t)blockIdx.y * a.D + dcol] = v;
  }
  if (dok) {
#pragma unroll
    for (int lt = 0; lt < LTM; ++lt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int l = 16 * lt + 4 * q + g;
        if (l < a.Lt) a.dW_slab[((int64_t)blockIdx.y * a.D + dcol) * a.Lt + l] = dwt[lt][g] * inv_e;
      }
  }
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
  pl.nblk = (N + 63) / 64;
  pl.GS = 4;
  int64_t S = (1536 + pl.nblk * E - 1) / (pl.nblk * E);
  const int64_t smax = (D + 128 * pl.GS - 1) / (128 * pl.GS);
  if (S > smax) S = smax;
  if (S > 32) S = 32;
  if (S < 1) S = 1;
  pl.S = (int)S;
  const int64_t gblk = (D + 63) / 64;
  int64_t SN = (1024 + gblk - 1) / gblk;
  if (SN > (N + 511) / 512) SN = (N + 511) / 512;
  if (SN > 16) SN = 16;
  if (SN < 1) SN = 1;
  pl.SN = (int)SN;
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
  constexpr int LP = 16 * ((KS + 3) / 4);
  const size_t lds = sizeof(float) * 2 * ((size_t)(a.E < NEG ? a.E : NEG) * LP * 68 + 64);
  // the opt-in above 64 KB is per kernel function and device and is set once: to the most the kernel can need
  constexpr size_t lds_max = sizeof(float) * 2 * ((size_t)NEG * LP * 68 + 64);
  static_assert(lds_max <= 160 * 1024, "nb_gene_kernel: LDS of the largest sample group");
  if (lds_max > 64 * 1024) {
    static bool set[64] = {};
    int dev = 0;
    GPZ_HIP_OK(hipGetDevice(&dev));
    if (!set[dev & 63]) {
      GPZ_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(nb_gene_kernel<KS>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
      set[dev & 63] = true;
    }
  }
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
