// nb_passes.h -- the two MFMA tile passes of the negative-binomial steps, once: nb.hip runs them with the counts as an
// operand, the zero part of nb_sparse.hip without.  Also what the dense count steps share on the host (the slice plan of
// both passes, pass B's LDS size and its opt-in) and in the terms of y and theta alone (digamma, the lgamma table's term).
//
// The layout of both passes -- which lane holds which element, how one product's accumulators are the next one's operand
// without a transpose through LDS, the double-buffered operands -- is poisson.hip's and is described there.  poisson.hip
// keeps its own text of the two kernels: its pass A runs two waves per SIMD on the 256-VGPR limit and any textual change
// re-rolls its register allocation ("Why the Poisson passes keep their own text").  The passes here are
// allocated for one wave per SIMD (pass A) and have room.
//
// A pass is a device function template over KS (k-steps of 4 factors), the policy P and the argument struct A, called from
// a thin __global__ kernel that carries the launch bounds.  A has the fields both steps name alike (W, V, theta, ith, expF,
// the slabs, D, Lt, E, S).  P supplies exactly what differs:
//   HAS_Y                      whether a count operand exists; spots(a), y(a): the spot extent (N or B) and the counts
//   SumsA, elem_a, fold_a      pass A's running sums of one 16-gene group, the element, and the group's term of the value
//   close_dv                   the closing scale of dV
//   SumsB, elem_b, fold_b      pass B's running sums of one tile, the element, and the tile's term of dtheta
// elem_* come in two forms, <false> for an interior tile and <true> for a masked one (ok: the element exists); they return
// E G, which replaces Z in the accumulator.
#pragma once
#include "common.h"
#include "mmops.h"
#include "vec.h"

namespace gpz {

constexpr float LN2 = 0.69314718055994530942f;
constexpr int PASS_EG = 4;      // samples pass B holds in LDS at a time (a "sample group")

// ---------------------------------------------------------------------------------------------------------------------
// host: slices and LDS
// ---------------------------------------------------------------------------------------------------------------------

struct SlicePlan { int S, GS, SN; int64_t nblk; };

// N spots (of the batch), D genes, E samples.  Pass A: enough (spot tile, gene slice) workgroups to fill 256 CUs a few times
// over, slices of >= 8 gene groups per wave.  Pass B: gene blocks of 64 x spot slices.
static SlicePlan slice_plan(int64_t N, int64_t D, int E) {
  SlicePlan pl;
  pl.nblk = (N + 63) / 64;                     // spot tiles of pass A
  pl.GS = 4;                                   // 16-gene sub-groups (waves) per workgroup
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
  return pl;
}

// bytes of pass B's dynamic LDS with sample groups of eg: exp(F) [2][eg][LP][68] and V [2][64]
constexpr size_t pass_b_lds(int KS, int eg) { return sizeof(float) * 2 * ((size_t)eg * (16 * ((KS + 3) / 4)) * 68 + 64); }

// The opt-in above 64 KB is per kernel function and device and is set ONCE, so it is set to what the kernel can need at most
// (a full sample group), not to one call's size: a later call with more samples must still fit under it.
template <auto Kernel>
static int lds_opt_in(size_t lds_max) {
  if (lds_max <= 64 * 1024) return 0;
  static bool set[64] = {};
  int dev = 0;
  GPZ_HIP_OK(hipGetDevice(&dev));
  if (!set[dev & 63]) {
    GPZ_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
    set[dev & 63] = true;
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// the terms of y and theta alone
// ---------------------------------------------------------------------------------------------------------------------

// psi(x), x > 0, fp64: the argument shifted above 6 by psi(x) = psi(x + 1) - 1 / x, then the asymptotic series (its first
// omitted term is below 1e-12 there)
__device__ __forceinline__ double digamma_pos(double x) {
  double r = 0.0;
  while (x < 6.0) { r -= 1.0 / x; x += 1.0; }
  const double i = 1.0 / x, i2 = i * i;
  const double ser = i2 * (1.0 / 12 - i2 * (1.0 / 120 - i2 * (1.0 / 252 - i2 * (1.0 / 240 - i2 * (1.0 / 132 - i2 * (691.0 / 32760 - i2 / 12))))));
  return r + log(x) - 0.5 * i - ser;
}

// lgamma(y + 1) of a count y != 0 with yi = (int)y, whole = (y is a positive integer): the entry of the workgroup's
// 256-entry table lfact[i] = lgammaf(i + 1) where there is one
__device__ __forceinline__ float lgamma1p_term(const float* lfact, float y, int yi, bool whole) {
  return (whole && yi < 256) ? lfact[yi] : lgammaf(y + 1.f);
}

// ---------------------------------------------------------------------------------------------------------------------
// Pass A  grid (E * ceil(spots/64), S), 4 waves; see spot_mfma_kernel of poisson.hip.
// ---------------------------------------------------------------------------------------------------------------------
template <int KS, typename P, typename A>
__device__ __forceinline__ void nb_pass_a(const A a, int GS) {
  constexpr int LT16 = (KS + 3) / 4;
  __shared__ double sh[8];
  const int64_t N = P::spots(a);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int e = blockIdx.x % a.E, gs = wave;
  const int s = blockIdx.y;
  const int64_t n0 = (int64_t)(blockIdx.x / a.E) * 64;
  const int64_t per = (int64_t)a.Lt * N;
  const int64_t dper = (a.D + a.S - 1) / a.S;
  const int64_t d_lo = s * dper, d_hi = (d_lo + dper < a.D) ? d_lo + dper : a.D;
  const float inv_e = 1.f / (float)a.E;
  const bool vec = (N & 3) == 0;
  const bool tile_full = n0 + 64 <= N;
  float vn[4], bz[KS][4];
  bool nok[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int64_t n = n0 + 4 * r + c;
    nok[c] = n < N;
    vn[c] = nok[c] ? a.V[n] : 1.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int l = 4 * ks + q;
      bz[ks][c] = (nok[c] && l < a.Lt) ? a.expF[e * per + (int64_t)l * N + n] : 0.f;
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
  // (1 for a gene that does not exist: its elements are masked, but the arithmetic must stay finite); yv only with counts
  struct Group { float wa[KS]; f32x4 yv[4]; float wt[4][LT16]; float th[4], ith[4]; };
  auto load_group = [&](int64_t d0, Group& G) __attribute__((always_inline)) {
    if constexpr (P::HAS_Y) {
      if (d0 + 16 <= d_hi && tile_full && vec) {       // interior: no masks, the counts 16 bytes at a time
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
          G.yv[g] = *reinterpret_cast<const f32x4*>(P::y(a) + dg * N + n0 + 4 * r);
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
      const bool ok = dg < d_hi;
      G.th[g] = ok ? a.theta[dg] : 1.f;
      G.ith[g] = ok ? a.ith[dg] : 1.f;
      if constexpr (P::HAS_Y) {
        G.yv[g] = f32x4{0, 0, 0, 0};
        if (ok) {
          const float* yp = P::y(a) + dg * N + n0 + 4 * r;
          if (vec && nok[3]) G.yv[g] = *reinterpret_cast<const f32x4*>(yp);
          else {
#pragma unroll
            for (int c = 0; c < 4; ++c) if (nok[c]) G.yv[g][c] = yp[c];
          }
        }
      }
#pragma unroll
      for (int lt = 0; lt < LT16; ++lt) {
        const int l = 16 * lt + r;
        G.wt[g][lt] = (ok && l < a.Lt) ? a.W[dg * a.Lt + l] : 0.f;
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
    // element-wise: the sample-dependent terms of the log-density, dV's sum, and E G in place of Z (1 / E applied at the end)
    typename P::SumsA sa;
    if (d0 + 16 <= d_hi && tile_full) {
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          float y1 = 0.f;
          if constexpr (P::HAS_Y) y1 = cur.yv[g][c];
          z[c][g] = P::template elem_a<false>(sa, g, z[c][g], y1, vn[c], cur.th[g], cur.ith[g], dv[c], true);
        }
    } else {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const bool dok = d0 + 4 * q + g < d_hi;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          float y1 = 0.f;
          if constexpr (P::HAS_Y) y1 = cur.yv[g][c];
          z[c][g] = P::template elem_a<true>(sa, g, z[c][g], y1, vn[c], cur.th[g], cur.ith[g], dv[c], dok && nok[c]);
        }
      }
    }
    ll += P::fold_a(sa, cur.th);
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
        float* dp = a.dexp_slab + ((slab * a.E + e) * a.Lt + l) * N + n0 + 4 * r;
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
    float v = P::close_dv(dv[c], vn[c], inv_e);
    v += __shfl_xor(v, 16); v += __shfl_xor(v, 32);
    if (q == 0 && nok[c]) a.dV_slab[((int64_t)s * nw + e * GS + gs) * N + n0 + 4 * r + c] = v;
  }
  const double t = block_sum(ll * (double)inv_e, sh);
  if (threadIdx.x == 0) a.ll_slab[(int64_t)s * gridDim.x + blockIdx.x] = t;
}

// ---------------------------------------------------------------------------------------------------------------------
// Pass B  grid (ceil(D/64), SN), 4 waves, pass_b_lds bytes of dynamic LDS; see gene_mfma_kernel of poisson.hip.  This
// lane's gene is column r of the transposed tile, so theta is one register, and dtheta's sample-dependent sum reduces over
// the same axes as dW: one more output column per gene.
// ---------------------------------------------------------------------------------------------------------------------
template <int KS, typename P, typename A>
__device__ __forceinline__ void nb_pass_b(const A a, int SN) {
  constexpr bool TAIL = (KS % 4) == 1;
  constexpr int LTM = TAIL ? KS / 4 : (KS + 3) / 4, LTA = LTM > 0 ? LTM : 1, L0 = 16 * LTM;
  constexpr int LT16 = (KS + 3) / 4, LP = 16 * LT16, PF = 68;
  extern __shared__ float smem_pass_b[];
  const int64_t N = P::spots(a);
  const int EG = a.E < PASS_EG ? a.E : PASS_EG, NG = (a.E + EG - 1) / EG;
  const int FB = EG * LP * PF;
  float* sF = smem_pass_b;                      // [2][EG][LP][PF]
  float* sV = smem_pass_b + 2 * FB;             // [2][64]
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int64_t d0 = ((int64_t)blockIdx.x * 4 + wave) * 16;
  const int64_t dcol = d0 + r;
  const bool dok = dcol < a.D;
  const bool d_full = d0 + 16 <= a.D;
  const int64_t ntiles = (N + 63) / 64, tper = (ntiles + SN - 1) / SN;
  const int64_t t_lo = blockIdx.y * tper, t_hi = (t_lo + tper < ntiles) ? t_lo + tper : ntiles;
  const float inv_e = 1.f / (float)a.E;
  const bool vec = (N & 3) == 0;
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
  double dth = 0.0;                             // dtheta's sample-dependent sum over this lane's spots and all samples
  const int arow = 16 * (r >> 2) + (r & 3);
  for (int i = threadIdx.x; i < 2 * FB; i += 256) sF[i] = 0.f;
  __syncthreads();
#if defined(__HIP_DEVICE_COMPILE__)
  typedef __attribute__((address_space(3))) void lds_void;
  const int64_t per = (int64_t)a.Lt * N;
  const __amdgpu_buffer_rsrc_t f_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.expF), 0, (int)((int64_t)a.E * per * sizeof(float)), 0x00020000);
  const __amdgpu_buffer_rsrc_t v_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.V), 0, (int)(N * sizeof(float)), 0x00020000);
#endif
  auto stage = [&](int64_t tt, int gi, int buf) __attribute__((always_inline)) {
#if defined(__HIP_DEVICE_COMPILE__)
    const int64_t n0 = tt * 64;
    const int e0 = gi * EG, ne = (a.E - e0 < EG) ? a.E - e0 : EG;
    for (int el = 0; el < ne; ++el)
      for (int l = wave; l < a.Lt; l += 4)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(f_rsrc, (lds_void*)(sF + buf * FB + (el * LP + l) * PF), 4, lane * 4,
                                                 (int)(((e0 + el) * per + (int64_t)l * N + n0) * 4), 0, 0);
    if (wave == 0)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(v_rsrc, (lds_void*)(sV + buf * 64), 4, lane * 4, (int)(n0 * 4), 0, 0);
#endif
  };
  auto load_y = [&](int64_t tt, f32x4 (&yv)[4]) __attribute__((always_inline)) {
    if constexpr (P::HAS_Y) {
      const int64_t n0 = tt * 64;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int64_t n = n0 + 16 * q + 4 * c;
        yv[c] = f32x4{0, 0, 0, 0};
        if (dok) {
          const float* yp = P::y(a) + dcol * N + n;
          if (vec && n + 3 < N) yv[c] = *reinterpret_cast<const f32x4*>(yp);
          else {
#pragma unroll
            for (int g = 0; g < 4; ++g) if (n + g < N) yv[c][g] = yp[g];
          }
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
        // E G^T in place of Z^T (1 / E applied at the end) and dtheta's term; a spot past the extent reads V = 0 or a
        // finite neighbour through the buffer descriptor, so the masked form replaces V as well as Z
        typename P::SumsB sb;
        if (d_full && n0 + 64 <= N) {
#pragma unroll
          for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              float y1 = 0.f;
              if constexpr (P::HAS_Y) y1 = yv[c][g];
              z[c][g] = P::template elem_b<false>(sb, z[c][g], y1, vv[c][g], ith, true);
            }
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              float y1 = 0.f;
              if constexpr (P::HAS_Y) y1 = yv[c][g];
              z[c][g] = P::template elem_b<true>(sb, z[c][g], y1, vv[c][g], ith, dok && n0 + 16 * q + 4 * c + g < N);
            }
        }
        dth += P::fold_b(sb, ith);              // fp32 sums of 16 terms, fp64 across tiles and samples
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
    if constexpr (P::HAS_Y) {
#pragma unroll
      for (int c = 0; c < 4; ++c) yv[c] = yn[c];
    }
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

}  // namespace gpz
