// nb_sparse.hip -- the negative-binomial step of nb.hip for counts stored as their non-zeros (SparseCounts): the same
// log-likelihood and the same five gradients on a batch of B spots, and nothing of D x B elements is read, written or
// allocated.
//
// Notation of nb.hip: mu = V[n] Z[e,d,n], Z = sum_l W[d,l] expF[e,l,n], x = mu / theta[d], u = 1 + x.  The log-density
//   ll = y log x - (y + theta) log1p(x) + [lgamma(y + theta) - lgamma(theta)] - lgamma(y + 1)
// splits into a part that needs no y and a part that vanishes where y = 0:
//   ll = { -theta log1p(x) }  +  { y log(mu / (mu + theta)) + lgamma(y + theta) - lgamma(theta) - lgamma(y + 1) }.
//
// ZERO PART, over every (e, d, n) of the batch (the step of nb.hip on y = 0; log1p compensated as there):
//   ll0        = -theta log1p(x),   log1p(x) = log(u) + (x - (u - 1)) / u
//   E G0       = -V / u                                   (d ll0 / d Z; no reciprocal of Z: -mu / (u Z) = -V / u)
//   dV0[n]     = (1/E) sum_{e,d} -Z / u
//   dtheta0[d] = (1/E) sum_{e,n} ( -log1p(x) + x / u )
//   dW0 = G0 expF^T,  dexpF0 = W^T G0                     (the two MFMA products of nb.hip's passes)
// NON-ZERO PART, for each stored entry k = (d, n) of the batch with count y != 0, r = 1 / (mu + theta):
//   value    += (1/E) sum_e y log(mu r)  +  lgamma(y + theta) - lgamma(theta);        loglik[1] += lgamma(y + 1)
//   E dG      = y theta r / Z  ->  dW[d,l] += (1/E) sum_e dG expF[e,l,n],   dexpF[e,l,n] += (1/E) dG W[d,l]
//   dV[n]    += (1/E) sum_e y theta r / V[n]
//   dtheta[d]+= psi(y + theta) - psi(theta)  -  (1/E) sum_e y r
// and dmean = sum_e dexpF expF, dscale = sum_e dexpF expF eps over the sum of both parts.  A stored zero adds exactly 0.
//
// Launches (fp32, fp64 for the scalars, the per-gene constants and dtheta; no atomics, no workgroup waits on another,
// every sum in a fixed order -> two calls agree bit for bit):
//   nbs_prologue_kernel  expF (E,Lt,B) for the zero part; expF and expF eps transposed to [B][E][LT] for the non-zero part
//                        (LT = Lt padded to the kernel instance, zeros beyond Lt); 1 / theta
//   chunks_kernel        the gene pass's work list: row d is cut into ceil(len_d / 512) chunks of consecutive non-zeros
//   nbs_zspot_kernel     zero part, pass A of nb.hip without its y operand: value, dV0 and dexpF0 slabs
//   nbs_zgene_kernel     zero part, pass B of nb.hip without its y operand: dW0 slabs and dtheta0
//   nbs_spot_kernel      non-zero part, one wave per batch spot: value, dV and the dmean / dscale contributions
//   nbs_gene_kernel      non-zero part, one wave per (gene, chunk): dW partial, sum y r, and the terms of y and theta alone
//                        (nb_const_kernel's arithmetic over the chunk's stored entries that lie in the batch)
//   nbs_finish_kernel    adds the two parts: slabs first, then the non-zero part, chunks in chunk order
// The layouts are those of nb.hip (which lane holds which element of a rate tile) and of poisson_sparse.hip (the two
// orders of the counts, idx / pos of a batch, the chunk list) and are described there.  The zero part's two passes are the
// templates of nb_passes.h that nb.hip runs with counts, here under the policy without (ZeroPart); the chunk list, the load
// of a row of W and the wave sum are sparse_rows.h's.  Only poisson.hip keeps its own text of the passes: its pass A runs
// two waves per SIMD at the 256-VGPR limit and any textual change re-rolls its register allocation ("Why the
// Poisson passes keep their own text").  The gene pass forms Z again from W[d,:] and the spot's exp(F) run: the only
// arrays whose length depends on nnz are per chunk.
#include "common.h"
#include "mmops.h"
#include "nb_passes.h"
#include "sparse_rows.h"

namespace gpz {
namespace nbs {

constexpr int NMAXL = 64;   // factors
constexpr int NMAXE = 32;   // samples per call
constexpr int CHUNK = 512;          // non-zeros of one gene row per wave of the gene pass
constexpr int GROUP_FLOATS = 3072;  // LDS floats per wave of the spot pass: exp(F) and exp(F) eps of one sample group

struct Args {
  const float *mean, *scale, *eps, *W, *V, *theta;             // (Lt,B), (Lt,B), (E,Lt,B), (D,Lt), (B,), (D,)
  const int64_t* col_ptr; const int32_t* col_gene; const float* col_val;
  const int64_t* row_ptr; const int32_t* row_spot; const int32_t* row_perm;
  const int32_t *idx, *pos;
  // zero part
  float *expF, *ith;                                           // (E,Lt,B), (D,) = 1 / theta
  float* dexp_slab; float* dV_slab; double* ll_slab;           // [SD][E][Lt][B], [SV][B], [S][nblk * E]
  float* dW_slab; double* dth_slab;                            // [SN][D][Lt], [SN][D]
  // non-zero part
  float *expT, *xeT;                                           // [B][E][LT]
  float *dm_nz, *ds_nz, *dV_nz; double* ll_spot;               // (Lt,B), (Lt,B), (B,), (B,)
  int32_t *cstart, *chunk_gene;                                // [D + 1], [nchunks]
  float* part; double* cterm;                                  // [nchunks][LT]; [nchunks][4]: sum y r, cl, cpsi, lg
  float *dW, *dmean, *dscale, *dV, *dtheta; double* loglik;
  int64_t N, B, D, nnz, nchunks;
  int Lt, LT, E, EG, S, SD, SV, SN, with_lgamma;
};

__global__ __launch_bounds__(256) void nbs_prologue_kernel(Args a) {
  __shared__ float xt[NMAXL][65], et[NMAXL][65];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int e = blockIdx.x % a.E;
  const int64_t j0 = (int64_t)(blockIdx.x / a.E) * 64;
  const int64_t j = j0 + lane;
  for (int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x; d < a.D; d += (int64_t)gridDim.x * 256) a.ith[d] = 1.f / a.theta[d];
  for (int l = wave; l < a.LT; l += 4) {
    float x = 0.f, ep = 0.f;
    if (l < a.Lt && j < a.B) {
      const int64_t ln = (int64_t)l * a.B + j;
      ep = a.eps[(int64_t)e * a.Lt * a.B + ln];
      x = __expf(a.mean[ln] + a.scale[ln] * ep);
      a.expF[(int64_t)e * a.Lt * a.B + ln] = x;
    }
    xt[l][lane] = x;
    et[l][lane] = x * ep;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 64 * a.LT; i += 256) {
    const int jj = i / a.LT, l = i - jj * a.LT;
    if (j0 + jj < a.B) {
      const int64_t o = ((j0 + jj) * a.E + e) * a.LT + l;
      a.expT[o] = xt[l][jj];
      a.xeT[o] = et[l][jj];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// zero part
// ---------------------------------------------------------------------------------------------------------------------

// The element-wise part of both zero passes.  In: the rate factor zz = Z, V of the spot, 1 / theta of the gene.
//   ru = 1 / u, lu = log2(u), c = (x - (u - 1)) / u          log1p(x) = ln2 lu + c
// Two transcendentals per element; E G0 = -v ru, dV0's term is zz ru and dtheta0's is x ru - log1p(x).  u and c's numerator
// are formed in one rounding each, fma(mu, 1 / theta, 1) and fma(mu, 1 / theta, -(u - 1)); written out, because the results
// are held bit for bit and the compiler's own choice of form changes with the text around the element.
struct ZElem { float x, ru, lu, c; };
__device__ __forceinline__ ZElem z_elem(float zz, float v, float ith) {
  ZElem o;
  const float mu = v * zz;
  o.x = mu * ith;
  const float u = __builtin_fmaf(mu, ith, 1.f);
  o.ru = __builtin_amdgcn_rcpf(u);
  o.lu = __builtin_amdgcn_logf(u);
  o.c = __builtin_fmaf(mu, ith, -(u - 1.f)) * o.ru;
  return o;
}

// What nb_passes.h asks of a step: no count operand, the spot extent is the batch's.
struct ZeroPart {
  static constexpr bool HAS_Y = false;
  static __device__ __forceinline__ int64_t spots(const Args& a) { return a.B; }
  static __device__ __forceinline__ const float* y(const Args&) { return nullptr; }
  // pass A, value of gene g: -theta (ln2 sum lu + sum c), the two sums apart and combined per group; dv is sum_d Z / u
  struct SumsA { float la[4] = {0.f, 0.f, 0.f, 0.f}, lb[4] = {0.f, 0.f, 0.f, 0.f}; };
  template <bool MASKED>
  static __device__ __forceinline__ float elem_a(SumsA& s, int g, float z, float, float v, float, float ith, float& dv, bool ok) {
    if constexpr (!MASKED) {
      const ZElem o = z_elem(z, v, ith);
      s.la[g] += o.lu;
      s.lb[g] += o.c;
      dv = __builtin_fmaf(z, o.ru, dv);
      return -v * o.ru;
    } else {
      const float zz = ok ? z : 1.f;
      const ZElem o = z_elem(zz, v, ith);
      s.la[g] += ok ? o.lu : 0.f;
      s.lb[g] += ok ? o.c : 0.f;
      dv += ok ? zz * o.ru : 0.f;
      return ok ? -v * o.ru : 0.f;
    }
  }
  static __device__ __forceinline__ double fold_a(const SumsA& s, const float (&th)[4]) {
    float lg4 = 0.f;
#pragma unroll
    for (int g = 0; g < 4; ++g) lg4 = __builtin_fmaf(th[g], __builtin_fmaf(LN2, s.la[g], s.lb[g]), lg4);
    return -(double)lg4;
  }
  static __device__ __forceinline__ float close_dv(float dv, float, float inv_e) { return -dv * inv_e; }
  // pass B, dtheta0's term x / u - (ln2 lu + c): the three sums apart, combined per tile
  struct SumsB { float tpa = 0.f, tpb = 0.f, tpx = 0.f; };
  template <bool MASKED>
  static __device__ __forceinline__ float elem_b(SumsB& s, float z, float, float v, float ith, bool ok) {
    if constexpr (!MASKED) {
      const ZElem o = z_elem(z, v, ith);
      s.tpa += o.lu;
      s.tpb += o.c;
      s.tpx = __builtin_fmaf(o.x, o.ru, s.tpx);
      return -v * o.ru;
    } else {
      const float zz = ok ? z : 1.f, v1 = ok ? v : 1.f;
      const ZElem o = z_elem(zz, v1, ith);
      s.tpa += ok ? o.lu : 0.f;
      s.tpb += ok ? o.c : 0.f;
      s.tpx += ok ? o.x * o.ru : 0.f;
      return ok ? -v1 * o.ru : 0.f;
    }
  }
  static __device__ __forceinline__ double fold_b(const SumsB& s, float) { return (double)(s.tpx - __builtin_fmaf(LN2, s.tpa, s.tpb)); }
};

// Pass A  grid (E * ceil(B/64), S), 4 waves: nb_pass_a of nb_passes.h.
#ifndef GPZ_NBS_SPOT_WAVES
#define GPZ_NBS_SPOT_WAVES 1
#endif
template <int KS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(GPZ_NBS_SPOT_WAVES, GPZ_NBS_SPOT_WAVES))) void nbs_zspot_kernel(Args a, int GS) {
  nb_pass_a<KS, ZeroPart>(a, GS);
}

// Pass B  grid (ceil(D/64), SN), 4 waves: nb_pass_b of nb_passes.h.
template <int KS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 4))) void nbs_zgene_kernel(Args a, int SN) {
  nb_pass_b<KS, ZeroPart>(a, SN);
}

// ---------------------------------------------------------------------------------------------------------------------
// non-zero part
// ---------------------------------------------------------------------------------------------------------------------

// Spot pass.  4 waves per workgroup, wave = batch spot j (global spot n = idx[j]); sp_spot_kernel of poisson_sparse.hip
// with the gene's theta as one more gathered operand.  Per non-zero and sample:
//   Z = w . expF[e],  mu = V Z,  r = 1 / (mu + theta),  q = y theta r / Z,  A[l] += q expF[e,l],  B[l] += q expF[e,l] eps[e,l]
// value += y log(mu r), dV += y theta r / V, and w[l] A[l], w[l] B[l] go to the spot's dmean / dscale contributions.
template <int LT>
__global__ __launch_bounds__(256) void nbs_spot_kernel(Args a) {
  extern __shared__ float nbs_smem[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* sx = nbs_smem + wave * 2 * a.EG * LT;           // [EG][LT] exp(F)
  float* se = sx + a.EG * LT;                            // [EG][LT] exp(F) eps
  int64_t j = (int64_t)blockIdx.x * 4 + wave;
  const bool valid = j < a.B;
  if (!valid) j = a.B - 1;                               // same work, nothing written: every wave reaches every barrier
  const int64_t n = a.idx ? a.idx[j] : j;
  const int64_t k0 = a.col_ptr[n], k1 = a.col_ptr[n + 1];
  const float vn = a.V[j];
  const float inv_e = 1.f / (float)a.E;
  float dm[LT], ds[LT];
#pragma unroll
  for (int l = 0; l < LT; ++l) dm[l] = ds[l] = 0.f;
  double ll = 0.0;
  float dvs = 0.f;                                       // sum_k sum_e y theta r
  for (int e0 = 0; e0 < a.E; e0 += a.EG) {
    const int ne = a.E - e0 < a.EG ? a.E - e0 : a.EG;
    __syncthreads();                                     // the previous group has been read
    const float* gx = a.expT + (j * a.E + e0) * LT;
    const float* ge = a.xeT + (j * a.E + e0) * LT;
    for (int i = lane; i < ne * LT; i += 64) { sx[i] = gx[i]; se[i] = ge[i]; }
    __syncthreads();
    for (int64_t k = k0 + lane; k < k1; k += 64) {
      const float y = a.col_val[k];
      if (y == 0.f) continue;                            // an explicit zero: 0 log(.) is never formed
      const int d = a.col_gene[k];
      const float th = a.theta[d], yth = y * th;
      float w[LT], A[LT], Bv[LT];
      load_w<LT>(a.W, d, a.Lt, w);
#pragma unroll
      for (int l = 0; l < LT; ++l) A[l] = Bv[l] = 0.f;
      float slog = 0.f, sr = 0.f;
      for (int e = 0; e < ne; ++e) {
        const f32x4* xp = reinterpret_cast<const f32x4*>(sx + e * LT);
        const f32x4* ep = reinterpret_cast<const f32x4*>(se + e * LT);
        float z = 0.f;
#pragma unroll
        for (int l = 0; l < LT; l += 4) {
          const f32x4 x = xp[l / 4];
          z = __builtin_fmaf(w[l], x[0], z); z = __builtin_fmaf(w[l + 1], x[1], z);
          z = __builtin_fmaf(w[l + 2], x[2], z); z = __builtin_fmaf(w[l + 3], x[3], z);
        }
        const float mu = vn * z;
        const float r = __builtin_amdgcn_rcpf(mu + th);
        slog += __logf(mu * r);
        sr += r;
        const float q = yth * r * __builtin_amdgcn_rcpf(z);
#pragma unroll
        for (int l = 0; l < LT; l += 4) {
          const f32x4 x = xp[l / 4], xe = ep[l / 4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            A[l + i] = __builtin_fmaf(q, x[i], A[l + i]);
            Bv[l + i] = __builtin_fmaf(q, xe[i], Bv[l + i]);
          }
        }
      }
      ll += (double)(y * slog);
      dvs = __builtin_fmaf(yth, sr, dvs);
#pragma unroll
      for (int l = 0; l < LT; ++l) {
        dm[l] = __builtin_fmaf(w[l], A[l], dm[l]);
        ds[l] = __builtin_fmaf(w[l], Bv[l], ds[l]);
      }
    }
  }
  // the wave owns its spot: reduce across the lanes in a fixed tree and write the spot's outputs directly
  float my_dm = 0.f, my_ds = 0.f;
#pragma unroll
  for (int l = 0; l < LT; ++l) {
    const float tm = wave_sum(dm[l]), ts = wave_sum(ds[l]);
    if (lane == l) { my_dm = tm; my_ds = ts; }
  }
  dvs = wave_sum(dvs);
  ll = wave_sum(ll);
  if (!valid) return;
  if (lane < a.Lt) {
    a.dm_nz[(int64_t)lane * a.B + j] = inv_e * my_dm;
    a.ds_nz[(int64_t)lane * a.B + j] = inv_e * my_ds;
  }
  if (lane == 0) {
    a.dV_nz[j] = inv_e * dvs / vn;
    a.ll_spot[j] = ll * (double)inv_e;
  }
}

// Gene pass.  4 waves per workgroup, wave = chunk w of the work list: at most 512 consecutive non-zeros of one gene row.
// The wave packs the chunk's entries that lie in the batch (pos[n] >= 0) and are not stored zeros into LDS, in their
// order, then every lane takes every 64th packed entry (sp_gene_kernel of poisson_sparse.hip).  The terms of y and theta
// alone follow nb_const_kernel of nb.hip: integer counts below 16 by the recurrences p_k = prod_{j<k} (theta + j),
// q_k = q_{k-1} (theta + k - 1) + p_{k-1} (sum 1 / (theta + k) = q_y / p_y, sum log(theta + k) = log p_y with the p_y
// multiplied up and the logarithm taken when the product leaves [1e-150, 1e150]); every other count is set aside into a
// second list in LDS while packing and worked off with all lanes busy (fp64 lgamma and the digamma series), lgamma(theta)
// and psi(theta) entering as one more entry of weight -count.
template <int LT>
__global__ __launch_bounds__(256) void nbs_gene_kernel(Args a) {
  __shared__ int32_t lj[4][CHUNK];
  __shared__ float ly[4][CHUNK];
  __shared__ float ls[4][CHUNK];
  __shared__ float lfact[256];
  lfact[threadIdx.x] = lgammaf((float)threadIdx.x + 1.f);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t wi = (int64_t)blockIdx.x * 4 + wave;
  const int g = wi < a.nchunks ? a.chunk_gene[wi] : -1;
  const float th = g >= 0 ? a.theta[g] : 1.f;
  const double thd = (double)th;
  const bool rec = thd > 1e-20 && thd < 1e8;
  int cnt = 0, scnt = 0;
  if (g >= 0) {
    const int64_t p0 = a.row_ptr[g] + (wi - a.cstart[g]) * CHUNK;
    const int64_t pe = a.row_ptr[g + 1], p1 = p0 + CHUNK < pe ? p0 + CHUNK : pe;
    for (int64_t pb = p0; pb < p1; pb += 64) {
      const int64_t p = pb + lane;
      int j = -1;
      float y = 0.f;
      if (p < p1) {
        const int n = a.row_spot[p];
        j = a.pos ? a.pos[n] : n;
        if (j >= 0) y = a.col_val[a.row_perm[p]];
      }
      const bool keep = j >= 0 && y != 0.f;
      const unsigned long long m = __ballot(keep);
      if (keep) {
        const int at = cnt + __popcll(m & ((1ull << lane) - 1ull));
        lj[wave][at] = j;
        ly[wave][at] = y;
      }
      cnt += __popcll(m);
      const int yi = (int)y;
      const bool aside = keep && !(y == (float)yi && yi > 0 && yi < 16 && rec);
      const unsigned long long ms = __ballot(aside);
      if (aside) ls[wave][scnt + __popcll(ms & ((1ull << lane) - 1ull))] = y;
      scnt += __popcll(ms);
    }
  }
  __syncthreads();                 // every wave, with or without a chunk, arrives here exactly once
  if (g < 0) return;
  float w[LT], acc[LT];
  load_w<LT>(a.W, g, a.Lt, w);
#pragma unroll
  for (int l = 0; l < LT; ++l) acc[l] = 0.f;
  double syr = 0.0, cl = 0.0, cp = 0.0, lg = 0.0, run = 1.0;
  for (int i = lane; i < cnt; i += 64) {
    const int64_t j = lj[wave][i];
    const float y = ly[wave][i];
    const float vj = a.V[j], yth = y * th;
    const f32x4* xp = reinterpret_cast<const f32x4*>(a.expT + j * a.E * LT);
    float sr = 0.f;
    for (int e = 0; e < a.E; ++e, xp += LT / 4) {
      float x[LT];
      float z = 0.f;
#pragma unroll
      for (int l = 0; l < LT; l += 4) {
        const f32x4 v = xp[l / 4];
        x[l] = v[0]; x[l + 1] = v[1]; x[l + 2] = v[2]; x[l + 3] = v[3];
        z = __builtin_fmaf(w[l], v[0], z); z = __builtin_fmaf(w[l + 1], v[1], z);
        z = __builtin_fmaf(w[l + 2], v[2], z); z = __builtin_fmaf(w[l + 3], v[3], z);
      }
      const float r = __builtin_amdgcn_rcpf(__builtin_fmaf(vj, z, th));
      sr += r;
      const float q = yth * r * __builtin_amdgcn_rcpf(z);
#pragma unroll
      for (int l = 0; l < LT; ++l) acc[l] = __builtin_fmaf(q, x[l], acc[l]);
    }
    syr += (double)(y * sr);
    const int yi = (int)y;
    const bool whole = y == (float)yi && yi > 0;
    if (whole && yi < 16 && rec) {
      double p = thd, q = 1.0;
      for (int k = 1; k < yi; ++k) { const double f = thd + k; q = __builtin_fma(q, f, p); p *= f; }
      cp += q / p;
      run *= p;
      if (run > 1e150 || run < 1e-150) { cl += log(run); run = 1.0; }
    }
    if (a.with_lgamma) lg += (double)lgamma1p_term(lfact, y, yi, whole);
  }
  cl += log(run);
  if (scnt > 0) {
    for (int i = lane; i <= scnt; i += 64) {
      const bool last = i == scnt;              // lgamma(theta), psi(theta), once for all the entries
      const double yt = (last ? 0.0 : (double)ls[wave][i]) + thd;
      const double wgt = last ? -(double)scnt : 1.0;
      cl += wgt * lgamma(yt);
      cp += wgt * digamma_pos(yt);
    }
  }
  float mine = 0.f;
#pragma unroll
  for (int l = 0; l < LT; ++l) {
    const float t = wave_sum(acc[l]);
    if (lane == l) mine = t;
  }
  syr = wave_sum(syr); cl = wave_sum(cl); cp = wave_sum(cp); lg = wave_sum(lg);
  if (lane < LT) a.part[wi * LT + lane] = mine;
  if (lane == 0) {
    double* ct = a.cterm + wi * 4;
    ct[0] = syr; ct[1] = cl; ct[2] = cp; ct[3] = lg;
  }
}

// The two parts added in a fixed order: the zero part's slabs in slab order, then the non-zero part (a row's chunks in
// chunk order).  dmean, dscale (Lt,B), dV (B), dW (D,Lt), dtheta (D); workgroup 0 also adds the scalars.
__global__ __launch_bounds__(256) void nbs_finish_kernel(Args a, int nblk_spot) {
  __shared__ double sh[8];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t per = (int64_t)a.Lt * a.B;
  const float inv_e = 1.f / (float)a.E;
  if (i < per) {
    float dm = 0.f, ds = 0.f;
    for (int e = 0; e < a.E; ++e) {
      float dx = 0.f;
      for (int s = 0; s < a.SD; ++s) dx += a.dexp_slab[((int64_t)s * a.E + e) * per + i];
      const float dF = dx * a.expF[e * per + i];
      dm += dF;
      ds += dF * a.eps[e * per + i];
    }
    a.dmean[i] = dm + a.dm_nz[i];
    a.dscale[i] = ds + a.ds_nz[i];
  }
  if (i < a.B) {
    float dv = 0.f;
    for (int s = 0; s < a.SV; ++s) dv += a.dV_slab[(int64_t)s * a.B + i];
    a.dV[i] = dv + a.dV_nz[i];
  }
  const int64_t dl = a.D * a.Lt;
  for (int64_t j = i; j < dl; j += (int64_t)gridDim.x * 256) {
    const int64_t d = j / a.Lt;
    const int l = (int)(j - d * a.Lt);
    float w = 0.f, v = 0.f;
    for (int s = 0; s < a.SN; ++s) w += a.dW_slab[(int64_t)s * dl + j];
    for (int64_t c = a.cstart[d]; c < a.cstart[d + 1]; ++c) v += a.part[c * a.LT + l];
    a.dW[j] = w + v * inv_e;
  }
  for (int64_t d = i; d < a.D; d += (int64_t)gridDim.x * 256) {
    double t = 0.0, yr = 0.0, cp = 0.0;
    for (int s = 0; s < a.SN; ++s) t += a.dth_slab[(int64_t)s * a.D + d];
    for (int64_t c = a.cstart[d]; c < a.cstart[d + 1]; ++c) { yr += a.cterm[c * 4]; cp += a.cterm[c * 4 + 2]; }
    a.dtheta[d] = (float)(t + (cp - yr * (double)inv_e));
  }
  if (blockIdx.x == 0) {
    double v = 0.0, vs = 0.0, vc = 0.0, vg = 0.0;
    for (int j = threadIdx.x; j < a.S * nblk_spot; j += 256) v += a.ll_slab[j];
    for (int64_t j = threadIdx.x; j < a.B; j += 256) vs += a.ll_spot[j];
    const int64_t used = a.cstart[a.D];
    for (int64_t c = threadIdx.x; c < used; c += 256) { vc += a.cterm[c * 4 + 1]; vg += a.cterm[c * 4 + 3]; }
    const double t = block_sum(v, sh);
    const double ts = block_sum(vs, sh);
    const double tc = block_sum(vc, sh);
    const double tg = block_sum(vg, sh);
    if (threadIdx.x == 0) { a.loglik[0] = (t + ts) + tc; a.loglik[1] = tg; }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------

// k-steps of 4 factors of the zero part's kernel instance (nb_ksteps of nb.hip): 1 .. 4, 5 .. 8, 9 .. 16, 17 .. 20, 21 .. 24,
// 25 .. 32, 33 .. 40, 41 .. 48 and 49 .. 64 factors
static int zero_ksteps(int Lt) {
  const int k = (Lt + 3) / 4;
  if (k <= 2) return k;
  if (k <= 4) return 4;
  if (k <= 6) return k;
  if (k <= 8) return 8;
  if (k <= 10) return 10;
  if (k <= 12) return 12;
  return 16;
}

// padded factor count of the non-zero part's kernel instance (sp_instance of poisson_sparse.hip)
static int nz_instance(int Lt) {
  const int sizes[] = {4, 8, 12, 16, 20, 24, 32, 40, 48, 64};
  for (int s : sizes) if (Lt <= s) return s;
  return 0;
}

static int nz_group(int LT, int E) {
  int g = GROUP_FLOATS / (2 * LT);
  if (g > NMAXE) g = NMAXE;
  if (g > E) g = E;
  return g < 1 ? 1 : g;
}

struct Plan { int S, GS, SN, LT, EG; int64_t nblk, nchunks; size_t bytes; };

static Plan make_plan(int64_t B, int64_t D, int Lt, int E, int64_t nnz, Args* a, void* ws) {
  Plan pl;
  const SlicePlan sp = slice_plan(B, D, E);
  pl.S = sp.S; pl.GS = sp.GS; pl.SN = sp.SN; pl.nblk = sp.nblk;
  pl.LT = nz_instance(Lt);
  pl.EG = nz_group(pl.LT, E);
  pl.nchunks = D + nnz / CHUNK;              // sum_d ceil(len_d / C) <= D + floor(nnz / C)
  Carver c(ws);
  float* expF = c.take<float>((size_t)E * Lt * B);
  float* ith = c.take<float>((size_t)D);
  float* dexp = c.take<float>((size_t)pl.S * pl.GS * E * Lt * B);
  float* dVs = c.take<float>((size_t)pl.S * E * pl.GS * B);
  float* dWs = c.take<float>((size_t)pl.SN * D * Lt);
  double* ll = c.take<double>((size_t)pl.S * pl.nblk * E);
  double* dth = c.take<double>((size_t)pl.SN * D);
  float* expT = c.take<float>((size_t)B * E * pl.LT);
  float* xeT = c.take<float>((size_t)B * E * pl.LT);
  float* dm_nz = c.take<float>((size_t)Lt * B);
  float* ds_nz = c.take<float>((size_t)Lt * B);
  float* dV_nz = c.take<float>((size_t)B);
  double* ll_spot = c.take<double>((size_t)B);
  int32_t* cstart = c.take<int32_t>((size_t)D + 1);
  int32_t* chunk_gene = c.take<int32_t>((size_t)pl.nchunks);
  float* part = c.take<float>((size_t)pl.nchunks * pl.LT);
  double* cterm = c.take<double>((size_t)pl.nchunks * 4);
  pl.bytes = c.used();
  if (a) {
    a->expF = expF; a->ith = ith; a->dexp_slab = dexp; a->dV_slab = dVs; a->dW_slab = dWs; a->ll_slab = ll; a->dth_slab = dth;
    a->expT = expT; a->xeT = xeT; a->dm_nz = dm_nz; a->ds_nz = ds_nz; a->dV_nz = dV_nz; a->ll_spot = ll_spot;
    a->cstart = cstart; a->chunk_gene = chunk_gene; a->part = part; a->cterm = cterm;
    a->S = pl.S; a->SD = pl.S * pl.GS; a->SV = pl.S * E * pl.GS; a->SN = pl.SN; a->LT = pl.LT; a->EG = pl.EG;
    a->nchunks = pl.nchunks;
  }
  return pl;
}

static int check_shape(const char* who, int64_t N, int64_t B, int64_t D, int Lt, int E, int64_t nnz) {
  GPZ_REQUIRE(N >= 1 && B >= 1 && D >= 1 && nnz >= 0, "%s: bad extents (N = %lld, B = %lld, D = %lld, nnz = %lld)", who,
              (long long)N, (long long)B, (long long)D, (long long)nnz);
  GPZ_REQUIRE(B <= N, "%s: a batch of %lld distinct spots out of %lld", who, (long long)B, (long long)N);
  GPZ_REQUIRE(Lt >= 1 && Lt <= NMAXL, "%s: %d factors unsupported (1..%d)", who, Lt, NMAXL);
  GPZ_REQUIRE(E >= 1 && E <= NMAXE, "%s: %d samples per call unsupported (1..%d)", who, E, NMAXE);
  GPZ_REQUIRE(N < (1ll << 31) && D < (1ll << 31) && nnz < (1ll << 31) && D + nnz / CHUNK < (1ll << 31),
              "%s: spots, genes and non-zeros are indexed with 32 bits", who);
  // nbs_zgene_kernel addresses exp(F) through a buffer descriptor with 32-bit byte extents and offsets
  GPZ_REQUIRE((int64_t)E * Lt * B * 4 < (1ll << 31),
              "%s: E * Lt * B = %lld elements of exp(F) exceed the 2 GiB a call can address: split the batch", who,
              (long long)((int64_t)E * Lt * B));
  return 0;
}

template <int KS>
static int zero_passes(const Args& a, const Plan& pl, hipStream_t s) {
  const size_t lds = pass_b_lds(KS, a.E < PASS_EG ? a.E : PASS_EG);
  static_assert(pass_b_lds(KS, PASS_EG) <= 160 * 1024, "nbs_zgene_kernel: LDS of the largest sample group");
  if (int rc = lds_opt_in<nbs_zgene_kernel<KS>>(pass_b_lds(KS, PASS_EG))) return rc;
  hipLaunchKernelGGL((nbs_zspot_kernel<KS>), dim3((unsigned)(pl.nblk * a.E), (unsigned)pl.S), dim3(64 * pl.GS), 0, s, a, pl.GS);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL((nbs_zgene_kernel<KS>), dim3((unsigned)((a.D + 63) / 64), (unsigned)pl.SN), dim3(256), lds, s, a, pl.SN);
  GPZ_LAUNCH_OK();
  return 0;
}

template <int LT>
static int nz_passes(const Args& a, hipStream_t s) {
  const size_t lds = sizeof(float) * ((size_t)4 * 2 * a.EG * LT);
  hipLaunchKernelGGL((nbs_spot_kernel<LT>), dim3((unsigned)((a.B + 3) / 4)), dim3(256), lds, s, a);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL((nbs_gene_kernel<LT>), dim3((unsigned)((a.nchunks + 3) / 4)), dim3(256), 0, s, a);
  GPZ_LAUNCH_OK();
  return 0;
}

}  // namespace nbs
}  // namespace gpz

using namespace gpz;
using namespace gpz::nbs;

extern "C" int gpz_nb_nsf_sparse_plan(int64_t N, int64_t B, int64_t D, int32_t Lt, int32_t E, int64_t nnz, int32_t* gene_chunk,
                                      int64_t* n_gene_chunks, int32_t* factors_padded, int32_t* zero_factors_padded,
                                      int32_t* gene_slices, int32_t* spot_slices, int32_t* samples_per_group,
                                      int32_t* zero_samples_per_group) {
  if (int rc = check_shape("gpz_nb_nsf_sparse_plan", N, B, D, Lt, E, nnz)) return rc;
  const Plan p = make_plan(B, D, Lt, E, nnz, nullptr, nullptr);
  if (gene_chunk) *gene_chunk = CHUNK;
  if (n_gene_chunks) *n_gene_chunks = p.nchunks;
  if (factors_padded) *factors_padded = p.LT;
  if (zero_factors_padded) *zero_factors_padded = 4 * zero_ksteps(Lt);
  if (gene_slices) *gene_slices = p.S;
  if (spot_slices) *spot_slices = p.SN;
  if (samples_per_group) *samples_per_group = p.EG;
  if (zero_samples_per_group) *zero_samples_per_group = E < PASS_EG ? E : PASS_EG;
  return 0;
}

extern "C" size_t gpz_nb_nsf_sparse_workspace_bytes(int64_t N, int64_t B, int64_t D, int64_t nnz, int32_t Lt, int32_t E) {
  if (check_shape("gpz_nb_nsf_sparse_workspace_bytes", N, B, D, Lt, E, nnz)) return 0;
  return make_plan(B, D, Lt, E, nnz, nullptr, nullptr).bytes;
}

extern "C" int gpz_nb_nsf_sparse(const float* mean, const float* scale, const float* eps, const float* W, const float* V,
                                 const float* theta, const int64_t* col_ptr, const int32_t* col_gene, const float* col_val,
                                 const int64_t* row_ptr, const int32_t* row_spot, const int32_t* row_perm,
                                 const int32_t* idx, const int32_t* pos, int64_t N, int64_t B, int64_t D, int64_t nnz,
                                 int32_t Lt, int32_t E, int32_t with_lgamma, double* loglik, float* dmean, float* dscale,
                                 float* dW, float* dV, float* dtheta, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_shape("gpz_nb_nsf_sparse", N, B, D, Lt, E, nnz)) return rc;
  GPZ_REQUIRE(mean && scale && eps && W && V && theta && col_ptr && row_ptr && loglik && dmean && dscale && dW && dV &&
              dtheta && ws, "gpz_nb_nsf_sparse: null pointer");
  GPZ_REQUIRE(nnz == 0 || (col_gene && col_val && row_spot && row_perm), "gpz_nb_nsf_sparse: null pointer (non-zeros)");
  GPZ_REQUIRE((idx == nullptr) == (pos == nullptr), "gpz_nb_nsf_sparse: idx and pos come together (both null: all spots)");
  GPZ_REQUIRE(idx || B == N, "gpz_nb_nsf_sparse: B = %lld of N = %lld spots needs idx and pos", (long long)B, (long long)N);
  {
    // the zero part moves rows of the batch arrays 16 bytes at a time, the non-zero part rows of W
    const void* arrays[] = {mean, scale, eps, W, V, theta, loglik, dmean, dscale, dW, dV, dtheta, ws};
    uintptr_t low = 0;
    for (const void* p : arrays) low |= reinterpret_cast<uintptr_t>(p);
    GPZ_REQUIRE((low & 15) == 0, "gpz_nb_nsf_sparse: every dense array argument and the workspace must be 16-byte aligned");
    GPZ_REQUIRE(((reinterpret_cast<uintptr_t>(idx) | reinterpret_cast<uintptr_t>(pos)) & 3) == 0,
                "gpz_nb_nsf_sparse: idx and pos must be 4-byte aligned");
  }
  Args a;
  const Plan pl = make_plan(B, D, Lt, E, nnz, &a, ws);
  GPZ_REQUIRE(ws_bytes >= pl.bytes, "gpz_nb_nsf_sparse: workspace of %zu bytes, %zu needed", ws_bytes, pl.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  a.mean = mean; a.scale = scale; a.eps = eps; a.W = W; a.V = V; a.theta = theta;
  a.col_ptr = col_ptr; a.col_gene = col_gene; a.col_val = col_val;
  a.row_ptr = row_ptr; a.row_spot = row_spot; a.row_perm = row_perm; a.idx = idx; a.pos = pos;
  a.dW = dW; a.dmean = dmean; a.dscale = dscale; a.dV = dV; a.dtheta = dtheta; a.loglik = loglik;
  a.N = N; a.B = B; a.D = D; a.nnz = nnz; a.Lt = Lt; a.E = E; a.with_lgamma = with_lgamma;
  hipLaunchKernelGGL(nbs_prologue_kernel, dim3((unsigned)((B + 63) / 64 * E)), dim3(256), 0, s, a);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(chunks_kernel, dim3(1), dim3(1024), 0, s, row_ptr, D, a.nchunks, CHUNK, false, a.cstart, a.chunk_gene);
  GPZ_LAUNCH_OK();
  int rc;
  switch (zero_ksteps(Lt)) {
    case 1: rc = zero_passes<1>(a, pl, s); break;
    case 2: rc = zero_passes<2>(a, pl, s); break;
    case 4: rc = zero_passes<4>(a, pl, s); break;
    case 5: rc = zero_passes<5>(a, pl, s); break;
    case 6: rc = zero_passes<6>(a, pl, s); break;
    case 8: rc = zero_passes<8>(a, pl, s); break;
    case 10: rc = zero_passes<10>(a, pl, s); break;
    case 12: rc = zero_passes<12>(a, pl, s); break;
    default: rc = zero_passes<16>(a, pl, s); break;
  }
  if (rc) return rc;
  switch (a.LT) {
    case 4: rc = nz_passes<4>(a, s); break;
    case 8: rc = nz_passes<8>(a, s); break;
    case 12: rc = nz_passes<12>(a, s); break;
    case 16: rc = nz_passes<16>(a, s); break;
    case 20: rc = nz_passes<20>(a, s); break;
    case 24: rc = nz_passes<24>(a, s); break;
    case 32: rc = nz_passes<32>(a, s); break;
    case 40: rc = nz_passes<40>(a, s); break;
    case 48: rc = nz_passes<48>(a, s); break;
    default: rc = nz_passes<64>(a, s); break;
  }
  if (rc) return rc;
  int64_t tot = (int64_t)Lt * B;
  if (tot < 256) tot = 256;
  hipLaunchKernelGGL(nbs_finish_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, a, (int)(pl.nblk * E));
  GPZ_LAUNCH_OK();
  return 0;
}
