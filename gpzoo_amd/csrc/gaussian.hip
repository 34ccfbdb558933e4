// gaussian.hip -- exact expected Gaussian log-likelihood of the real-valued factor models (RSF, FA) and its gradients,
// fused so that neither the (D, N) residual nor its scaled copy ever exists in HBM.
//
// y (D,N) real, W (D,Lt) real, b (D,), sd (D,) > 0, q(F) = N(mean, scale^2) independent, mean and scale (Lt,N):
//   r[d,n]   = y[d,n] - b[d] - sum_l W[d,l] mean[l,n]          g = r / sd[d]^2
//   S[l]     = sum_n scale[l,n]^2     R[d] = sum_n r[d,n]^2     Q[d] = sum_l W[d,l]^2 S[l]
//   loglik   = sum_d [ -N (log(2 pi) / 2 + log sd[d]) - (R[d] + Q[d]) / (2 sd[d]^2) ]   = E_q[ sum log N(y | b + W F, sd^2) ]
//   dmean    = W^T g            dscale[l,n] = -scale[l,n] sum_d W[d,l]^2 / sd[d]^2
//   dW       = g mean^T - W S / sd^2        db = sum_n g        dsd = -N / sd + (R + Q) / sd^3
// There is no link function, hence no Monte-Carlo sample axis and no transcendental per element: the value is exact.
//
// Work split (fp32 operands, the dense products on v_mfma_f32_16x16x4_f32, every sum across tiles fp64 in a fixed
// order, no atomics, no workgroup waits on another -> two calls agree bit for bit):
//   gfa_sums_kernel    S[l] and c[l] = sum_d W[d,l]^2 / sd[d]^2 in fp64, one workgroup per factor
//   gfa_spot_kernel    pass A: residual tiles with genes as rows -> dmean = W^T G partial slabs (gradient calls only)
//   gfa_gene_kernel    pass B: the transposed tiles (spots as rows) -> r mean^T, sum_n r and R per gene, partial slabs
//   gfa_finish_kernel  sums the slabs in order; dmean, dscale, dW, db, dsd, R and the per-gene log-likelihood in fp64
//   gfa_total_kernel   the scalar
// y is read twice in a gradient call (once per pass) and once in a value-only call (pass B alone).  The layout of the
// two passes -- which lane holds which element, how the residual tile is the next product's operand without a
// transpose through LDS -- is poisson.hip's and is described there.  1 / sd^2 depends on the gene only: pass B, where a
// lane's accumulators belong to one gene, leaves it to the finish kernel (in fp64); pass A applies it to the tile.
#include "common.h"
#include "mmops.h"

namespace gpz {
namespace gfa {

constexpr int GMAXL = 64;   // factors (spatial + non-spatial)

struct GfaArgs {
  const float* mean; const float* scale; const float* W; const float* b; const float* sd; const float* y;
  float* dmean_slab;                           // [SD][Lt][N]
  float* dW_slab; double* R_slab; double* rs_slab;   // [SN][D][Lt], [SN][D], [SN][D]
  double* SL; double* CL; double* llg;         // (64,), (64,), (D,)
  double* loglik; double* sse;
  float* dmean; float* dscale; float* dW; float* db; float* dsd;
  int64_t N, D;
  int Lt, S, SD, SN, grads;
};

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// S[l] = sum_n scale^2 and c[l] = sum_d W^2 / sd^2: grid (Lt), 1024 threads (there are only Lt workgroups: a thread's
// serial walk over N and D is the kernel's time), fp64 in a fixed order
__global__ __launch_bounds__(1024) void gfa_sums_kernel(GfaArgs a) {
  __shared__ double sh[16];
  const int l = blockIdx.x;
  double s = 0.0, c = 0.0;
  for (int64_t n = threadIdx.x; n < a.N; n += 1024) {
    const double v = (double)a.scale[(int64_t)l * a.N + n];
    s += v * v;
  }
  for (int64_t d = threadIdx.x; d < a.D; d += 1024) {
    const double w = (double)a.W[d * a.Lt + l], sd = (double)a.sd[d];
    c += w * w / (sd * sd);
  }
  const double ts = block_sum(s, sh);
  const double tc = block_sum(c, sh);
  if (threadIdx.x == 0) { a.SL[l] = ts; a.CL[l] = tc; }
}

// Pass A  grid (ceil(N/64), S), 4 waves: wave gs takes every 4th 16-gene group of gene slice s for the 64 spots of the
//         block; see spot_mfma_kernel of poisson.hip.  The B operand of the first product is `mean` itself.
//         Up to 32 factors the operands of two gene groups fit the 256 registers of two waves per SIMD; beyond that the
//         allocation is made for one wave per SIMD (the two-wave build spills 14 .. 118 registers per lane).
template <int KS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(KS > 8 ? 1 : 2, KS > 8 ? 1 : 2))) void gfa_spot_kernel(GfaArgs a, int GS) {
  constexpr int LT16 = (KS + 3) / 4;          // 16-row tiles of the factor axis
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int gs = wave, s = blockIdx.y;
  const int64_t n0 = (int64_t)blockIdx.x * 64;
  const int64_t dper = (a.D + a.S - 1) / a.S;
  const int64_t d_lo = s * dper, d_hi = (d_lo + dper < a.D) ? d_lo + dper : a.D;
  const bool vec = (a.N & 3) == 0;            // rows of y / the slabs start 16-byte aligned
  const bool tile_full = n0 + 64 <= a.N;      // (wave-uniform) every spot of the tile exists
  // this lane's four spots and the operand of the first product: B[k = factor 4s + q][column = spot 4r + c]
  float bz[KS][4];
  bool nok[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int64_t n = n0 + 4 * r + c;
    nok[c] = n < a.N;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int l = 4 * ks + q;
      bz[ks][c] = (nok[c] && l < a.Lt) ? a.mean[(int64_t)l * a.N + n] : 0.f;
    }
  }
  f32x4 dacc[LT16][4];
#pragma unroll
  for (int lt = 0; lt < LT16; ++lt)
#pragma unroll
    for (int c = 0; c < 4; ++c) dacc[lt][c] = f32x4{0, 0, 0, 0};
  // One 16-gene group's operands: W as the A operand of the first product (rows = genes r); y rows, b and 1 / sd^2 of
  // the genes 4q + g; W again as the A operand of W^T G (k slot q <-> gene 4q + g, rows = factors).  The next group's
  // loads are issued before the current group is computed.
  struct Group { float wa[KS]; f32x4 yv[4]; float bq[4], iv[4]; float wt[4][LT16]; };
  auto load_group = [&](int64_t d0, Group& G) __attribute__((always_inline)) {
    if (d0 + 16 <= d_hi && tile_full && vec) {      // interior: every address is valid, no branch per access
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
        G.bq[g] = a.b[dg];
        const float sd = a.sd[dg];
        G.iv[g] = 1.f / (sd * sd);
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
      G.bq[g] = 0.f;
      G.iv[g] = 0.f;
      if (dg < d_hi) {
        const float* yp = a.y + dg * a.N + n0 + 4 * r;
        if (vec && nok[3]) G.yv[g] = *reinterpret_cast<const f32x4*>(yp);
        else {
#pragma unroll
          for (int c = 0; c < 4; ++c) if (nok[c]) G.yv[g][c] = yp[c];
        }
        G.bq[g] = a.b[dg];
        const float sd = a.sd[dg];
        G.iv[g] = 1.f / (sd * sd);
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
    // predicted tile (W mean)[gene][spot]
    f32x4 z[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      z[c] = f32x4{0, 0, 0, 0};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) z[c] = mfma4(cur.wa[ks], bz[ks][c], z[c]);
    }
    // G = (y - b - W mean) / sd^2 in place (gene rows on the register axis); genes past the slice have iv = 0 and
    // finite operands, spots past N are masked
    if (tile_full) {
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int c = 0; c < 4; ++c) z[c][g] = ((cur.yv[g][c] - cur.bq[g]) - z[c][g]) * cur.iv[g];
    } else {
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int c = 0; c < 4; ++c) z[c][g] = nok[c] ? ((cur.yv[g][c] - cur.bq[g]) - z[c][g]) * cur.iv[g] : 0.f;
    }
    // dmean[factor][spot] += sum over the group's genes: k-step g pairs G's register g (gene 4q + g) with
    // A[row = factor 16 lt + r][k slot q] = W[gene 4q + g][factor 16 lt + r]
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int lt = 0; lt < LT16; ++lt)
#pragma unroll
        for (int c = 0; c < 4; ++c) dacc[lt][c] = mfma4(cur.wt[g][lt], z[c][g], dacc[lt][c]);
    cur = nxt;
  }
  // one slab per (slice, gene sub-group); a wave without a group writes its zeros.  The finish kernel sums them in order.
  const int64_t slab = (int64_t)s * GS + gs;
#pragma unroll
  for (int lt = 0; lt < LT16; ++lt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int l = 16 * lt + 4 * q + g;
      if (l < a.Lt) {
        float* dp = a.dmean_slab + (slab * a.Lt + l) * a.N + n0 + 4 * r;
        if (vec && nok[3])
          *reinterpret_cast<f32x4*>(dp) = f32x4{dacc[lt][0][g], dacc[lt][1][g], dacc[lt][2][g], dacc[lt][3][g]};
        else {
#pragma unroll
          for (int c = 0; c < 4; ++c) if (nok[c]) dp[c] = dacc[lt][c][g];
        }
      }
    }
}

// Pass B  grid (ceil(D/64), SN), 4 waves: wave w owns the 16 genes 64 b + 16 w and sweeps spot slice sn in tiles of 64
//         (the `mean` tile staged in LDS, double buffered through registers; spots past N are staged as zeros).  The
//         tile is computed TRANSPOSED, spots as rows; see gene_mfma_kernel of poisson.hip.  The residual itself is the
//         operand of r mean^T; sum_n r and sum_n r^2 leave each tile as fp32 sums of 16 terms and are kept in fp64.
//         GRADS = false: the residual sums only (value-only calls).
template <int KS, bool GRADS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 4))) void gfa_gene_kernel(GfaArgs a, int SN) {
  constexpr int LT16 = (KS + 3) / 4, LP = 16 * LT16, PF = 68;      // factor rows staged (zero padded), row pitch
  constexpr int NST = LP / 4;                                        // rows a wave stages per tile
  __shared__ float sF[2 * LP * PF];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int64_t d0 = ((int64_t)blockIdx.x * 4 + wave) * 16;
  const int64_t dcol = d0 + r;                  // this lane's gene (a column of the transposed tile)
  const bool dok = dcol < a.D;
  const bool d_full = d0 + 16 <= a.D;           // (wave-uniform) every gene of this wave exists
  const int64_t ntiles = (a.N + 63) / 64, tper = (ntiles + SN - 1) / SN;
  const int64_t t_lo = blockIdx.y * tper, t_hi = (t_lo + tper < ntiles) ? t_lo + tper : ntiles;
  const bool vec = (a.N & 3) == 0;
  float wb[KS];                                 // B[k = factor 4s + q][column = gene r]
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int l = 4 * ks + q;
    wb[ks] = (dok && l < a.Lt) ? a.W[dcol * a.Lt + l] : 0.f;
  }
  const float bg = dok ? a.b[dcol] : 0.f;
  f32x4 dwt[LT16];
#pragma unroll
  for (int lt = 0; lt < LT16; ++lt) dwt[lt] = f32x4{0, 0, 0, 0};
  double rsum = 0.0, rsq = 0.0;
  const int arow = 16 * (r >> 2) + (r & 3);     // A row r of sub-tile c is spot 16 (r >> 2) + 4c + (r & 3) of the tile
  for (int i = threadIdx.x; i < 2 * LP * PF; i += 256) sF[i] = 0.f;      // the padded factor rows stay zero
  __syncthreads();
  // rows wave, wave + 4, ... of the tile: one 256-byte row of 64 spots per wave instruction
  auto stage_load = [&](int64_t tt, float (&st)[NST]) __attribute__((always_inline)) {
    const int64_t n = tt * 64 + lane;
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const int l = wave + 4 * i;
      st[i] = (l < a.Lt && n < a.N) ? a.mean[(int64_t)l * a.N + n] : 0.f;
    }
  };
  auto stage_write = [&](int buf, const float (&st)[NST]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const int l = wave + 4 * i;
      if (l < a.Lt) sF[buf * LP * PF + l * PF + lane] = st[i];
    }
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
  float st[NST];
  if (t_lo < t_hi) {
    stage_load(t_lo, st);
    load_y(t_lo, yv);
    stage_write(0, st);
  }
  __syncthreads();
  int buf = 0;
  for (int64_t tt = t_lo; tt < t_hi; ++tt, buf ^= 1) {
    const int64_t n0 = tt * 64;
    const bool more = tt + 1 < t_hi;
    if (more) { stage_load(tt + 1, st); load_y(tt + 1, yn); }
    const float* fe = sF + buf * LP * PF;
    f32x4 z[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      z[c] = f32x4{0, 0, 0, 0};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) z[c] = mfma4(fe[(4 * ks + q) * PF + arow + 4 * c], wb[ks], z[c]);
    }
    // the residual r^T in place; interior tiles without masks
    if (d_full && n0 + 64 <= a.N) {
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int g = 0; g < 4; ++g) z[c][g] = (yv[c][g] - bg) - z[c][g];
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const bool ok = dok && n0 + 16 * q + 4 * c + g < a.N;
          z[c][g] = ok ? (yv[c][g] - bg) - z[c][g] : 0.f;
        }
    }
    float p1 = 0.f, p2 = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int g = 0; g < 4; ++g) { p1 += z[c][g]; p2 = __builtin_fmaf(z[c][g], z[c][g], p2); }
    rsum += (double)p1;
    rsq += (double)p2;
    if constexpr (GRADS) {
      // (r mean^T)^T[factor][gene] += sum over the tile's spots: k-step (c, g) pairs r^T's register g of sub-tile c
      // (spot 16q + 4c + g) with A[row = factor 16 lt + r][k slot q] = mean[factor][that spot]
#pragma unroll
      for (int lt = 0; lt < LT16; ++lt)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const f32x4 fa = *reinterpret_cast<const f32x4*>(fe + (16 * lt + r) * PF + 16 * q + 4 * c);
#pragma unroll
          for (int g = 0; g < 4; ++g) dwt[lt] = mfma4(fa[g], z[c][g], dwt[lt]);
        }
    }
    if (more) {
      stage_write(buf ^ 1, st);
#pragma unroll
      for (int c = 0; c < 4; ++c) yv[c] = yn[c];
    }
    __syncthreads();        // the next tile has landed; every wave is done with this one's buffer
  }
  // the four spot groups of gene r (lanes r, r + 16, r + 32, r + 48) in a fixed order; lanes q == 0 write
  rsum += __shfl_xor(rsum, 16); rsum += __shfl_xor(rsum, 32);
  rsq += __shfl_xor(rsq, 16); rsq += __shfl_xor(rsq, 32);
  if (dok) {
    if (q == 0) {
      a.rs_slab[(int64_t)blockIdx.y * a.D + dcol] = rsum;
      a.R_slab[(int64_t)blockIdx.y * a.D + dcol] = rsq;
    }
    if constexpr (GRADS) {
#pragma unroll
      for (int lt = 0; lt < LT16; ++lt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int l = 16 * lt + 4 * q + g;
          if (l < a.Lt) a.dW_slab[((int64_t)blockIdx.y * a.D + dcol) * a.Lt + l] = dwt[lt][g];
        }
    }
  }
}

// The slabs summed in order (fp64) and the closed-form terms.  grid covers max(Lt N, D Lt, D) elements.
__global__ __launch_bounds__(256) void gfa_finish_kernel(GfaArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t per = (int64_t)a.Lt * a.N, dl = a.D * a.Lt;
  if (a.grads && i < per) {
    double dm = 0.0;
    for (int s = 0; s < a.SD; ++s) dm += (double)a.dmean_slab[(int64_t)s * per + i];
    a.dmean[i] = (float)dm;
    a.dscale[i] = (float)(-(double)a.scale[i] * a.CL[i / a.N]);
  }
  if (a.grads && i < dl) {
    const int64_t d = i / a.Lt;
    const int l = (int)(i - d * a.Lt);
    const double sd = (double)a.sd[d], iv = 1.0 / (sd * sd);
    double w = 0.0;
    for (int s = 0; s < a.SN; ++s) w += (double)a.dW_slab[(int64_t)s * dl + i];
    a.dW[i] = (float)(iv * (w - (double)a.W[i] * a.SL[l]));
  }
  if (i < a.D) {
    const double sd = (double)a.sd[i], iv = 1.0 / (sd * sd);
    double R = 0.0, rs = 0.0, Q = 0.0;
    for (int s = 0; s < a.SN; ++s) { R += a.R_slab[(int64_t)s * a.D + i]; rs += a.rs_slab[(int64_t)s * a.D + i]; }
    for (int l = 0; l < a.Lt; ++l) {
      const double w = (double)a.W[i * a.Lt + l];
      Q += w * w * a.SL[l];
    }
    if (a.sse) a.sse[i] = R;
    a.llg[i] = -(double)a.N * (0.91893853320467274178 + log(sd)) - 0.5 * (R + Q) * iv;
    if (a.grads) {
      a.db[i] = (float)(rs * iv);
      a.dsd[i] = (float)(-(double)a.N / sd + (R + Q) * iv / sd);
    }
  }
}

__global__ __launch_bounds__(1024) void gfa_total_kernel(GfaArgs a) {
  __shared__ double sh[16];
  double v = 0.0;
  for (int64_t j = threadIdx.x; j < a.D; j += 1024) v += a.llg[j];
  const double t = block_sum(v, sh);
  if (threadIdx.x == 0) a.loglik[0] = t;
}

// k-steps of 4 factors of the kernel instance that serves Lt factors: poisson.hip's thirteen (1 .. 40 factors in steps
// of 4, then 48, 56 and 64)
static int gfa_ksteps(int Lt) {
  const int k = (Lt + 3) / 4;
  if (k <= 10) return k;
  if (k <= 12) return 12;
  if (k <= 14) return 14;
  return 16;
}

struct GfaPlan { int S, GS, SN; int64_t nblk; size_t bytes; float *dmean, *dWs; double *Rs, *rs, *SL, *CL, *llg; };

static GfaPlan gfa_plan(int64_t N, int64_t D, int Lt, void* partials) {
  GfaPlan pl;
  pl.nblk = (N + 63) / 64;                     // spot tiles of pass A
  pl.GS = 4;                                   // 16-gene sub-groups (waves) per workgroup
  // pass A: enough (spot tile, gene slice) workgroups to fill 256 CUs a few times over, slices of >= 8 gene groups per wave
  int64_t S = (1536 + pl.nblk - 1) / pl.nblk;
  const int64_t smax = (D + 128 * pl.GS - 1) / (128 * pl.GS);
  if (S > smax) S = smax;
  if (S > 32) S = 32;
  if (S < 1) S = 1;
  pl.S = (int)S;
  // pass B: gene blocks of 64 x spot slices
  const int64_t gblk = (D + 63) / 64;
  int64_t SN = (1024 + gblk - 1) / gblk;
  if (SN > (N + 511) / 512) SN = (N + 511) / 512;
  if (SN > 16) SN = 16;
  if (SN < 1) SN = 1;
  pl.SN = (int)SN;
  Carver c(partials);
  pl.dmean = c.take<float>((size_t)pl.S * pl.GS * Lt * N);
  pl.dWs = c.take<float>((size_t)pl.SN * D * Lt);
  pl.Rs = c.take<double>((size_t)pl.SN * D);
  pl.rs = c.take<double>((size_t)pl.SN * D);
  pl.SL = c.take<double>(GMAXL);
  pl.CL = c.take<double>(GMAXL);
  pl.llg = c.take<double>((size_t)D);
  pl.bytes = c.used();
  return pl;
}

static bool gfa_extents_ok(int64_t N, int64_t D, int Lt) {
  if (N < 1 || D < 1) { set_error("gpz_gaussian_fa: bad extents (N = %lld, D = %lld)", (long long)N, (long long)D); return false; }
  if (N >= (1ll << 31) || D >= (1ll << 31)) {
    set_error("gpz_gaussian_fa: N = %lld spots, D = %lld genes exceed the 2^31 - 1 a call can address", (long long)N, (long long)D);
    return false;
  }
  if (Lt < 1 || Lt > GMAXL) { set_error("gpz_gaussian_fa: %d factors unsupported (1..%d)", Lt, GMAXL); return false; }
  return true;
}

template <int KS>
static int gfa_passes(const GfaArgs& a, const GfaPlan& pl, hipStream_t s) {
  const dim3 ggrid((unsigned)((a.D + 63) / 64), (unsigned)pl.SN);
  if (a.grads) {
    hipLaunchKernelGGL((gfa_spot_kernel<KS>), dim3((unsigned)pl.nblk, (unsigned)pl.S), dim3(64 * pl.GS), 0, s, a, pl.GS);
    GPZ_LAUNCH_OK();
    hipLaunchKernelGGL((gfa_gene_kernel<KS, true>), ggrid, dim3(256), 0, s, a, pl.SN);
  } else {
    hipLaunchKernelGGL((gfa_gene_kernel<KS, false>), ggrid, dim3(256), 0, s, a, pl.SN);
  }
  GPZ_LAUNCH_OK();
  return 0;
}

}  // namespace gfa
}  // namespace gpz

using namespace gpz;
using namespace gpz::gfa;

extern "C" int gpz_gaussian_fa_plan(int64_t N, int64_t D, int32_t Lt, int32_t* factors_padded, int32_t* aligned_rows,
                                    int32_t* gene_slices, int32_t* spot_slices, int64_t* partials_bytes) {
  if (!gfa_extents_ok(N, D, Lt)) return -1;
  const GfaPlan pl = gfa_plan(N, D, Lt, nullptr);
  if (factors_padded) *factors_padded = 4 * gfa_ksteps(Lt);
  if (aligned_rows) *aligned_rows = (N & 3) == 0;
  if (gene_slices) *gene_slices = pl.S;
  if (spot_slices) *spot_slices = pl.SN;
  if (partials_bytes) *partials_bytes = (int64_t)pl.bytes;
  return 0;
}

extern "C" int gpz_gaussian_fa(const float* mean, const float* scale, const float* W, const float* b, const float* noise_sd,
                               const float* y, int64_t N, int64_t D, int32_t Lt, double* loglik, double* sse_per_gene,
                               float* dmean, float* dscale, float* dW, float* db, float* dnoise_sd,
                               void* partials, size_t partials_bytes, void* stream) {
  GPZ_REQUIRE(mean && scale && W && b && noise_sd && y && loglik && partials, "gpz_gaussian_fa: null pointer");
  const int ngrad = (dmean != nullptr) + (dscale != nullptr) + (dW != nullptr) + (db != nullptr) + (dnoise_sd != nullptr);
  GPZ_REQUIRE(ngrad == 0 || ngrad == 5, "gpz_gaussian_fa: the five gradient pointers must be all null or all set");
  {
    const void* arrays[] = {mean, scale, W, b, noise_sd, y, loglik, sse_per_gene, dmean, dscale, dW, db, dnoise_sd, partials};
    uintptr_t low = 0;
    for (const void* p : arrays) low |= reinterpret_cast<uintptr_t>(p);
    GPZ_REQUIRE((low & 15) == 0, "gpz_gaussian_fa: every array argument and partials must be 16-byte aligned");
  }
  if (!gfa_extents_ok(N, D, Lt)) return -1;
  GfaPlan pl = gfa_plan(N, D, Lt, partials);
  GPZ_REQUIRE(partials_bytes >= pl.bytes, "gpz_gaussian_fa: partials too small (%zu bytes, %zu needed)", partials_bytes, pl.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  GfaArgs a;
  a.mean = mean; a.scale = scale; a.W = W; a.b = b; a.sd = noise_sd; a.y = y;
  a.dmean_slab = pl.dmean; a.dW_slab = pl.dWs; a.R_slab = pl.Rs; a.rs_slab = pl.rs; a.SL = pl.SL; a.CL = pl.CL; a.llg = pl.llg;
  a.loglik = loglik; a.sse = sse_per_gene;
  a.dmean = dmean; a.dscale = dscale; a.dW = dW; a.db = db; a.dsd = dnoise_sd;
  a.N = N; a.D = D; a.Lt = Lt; a.S = pl.S; a.SD = pl.S * pl.GS; a.SN = pl.SN; a.grads = ngrad == 5;
  hipLaunchKernelGGL(gfa_sums_kernel, dim3((unsigned)Lt), dim3(1024), 0, s, a);
  GPZ_LAUNCH_OK();
  int rc;
  switch (gfa_ksteps(Lt)) {
    case 1: rc = gfa_passes<1>(a, pl, s); break;
    case 2: rc = gfa_passes<2>(a, pl, s); break;
    case 3: rc = gfa_passes<3>(a, pl, s); break;
    case 4: rc = gfa_passes<4>(a, pl, s); break;
    case 5: rc = gfa_passes<5>(a, pl, s); break;
    case 6: rc = gfa_passes<6>(a, pl, s); break;
    case 7: rc = gfa_passes<7>(a, pl, s); break;
    case 8: rc = gfa_passes<8>(a, pl, s); break;
    case 9: rc = gfa_passes<9>(a, pl, s); break;
    case 10: rc = gfa_passes<10>(a, pl, s); break;
    case 12: rc = gfa_passes<12>(a, pl, s); break;
    case 14: rc = gfa_passes<14>(a, pl, s); break;
    default: rc = gfa_passes<16>(a, pl, s); break;
  }
  if (rc) return rc;
  int64_t tot = a.grads ? (int64_t)Lt * N : D;
  if (a.grads && D * Lt > tot) tot = D * Lt;
  if (D > tot) tot = D;
  hipLaunchKernelGGL(gfa_finish_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, a);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(gfa_total_kernel, dim3(1), dim3(1024), 0, s, a);
  GPZ_LAUNCH_OK();
  return 0;
}
