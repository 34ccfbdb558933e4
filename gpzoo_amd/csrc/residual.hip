// residual.hip -- residuals of counts under the predictive mean rate of a fitted NSF factor model, and Moran's I of every
// gene's residuals over the spots' K-neighbour graph: is spatial structure left in what the model did not explain, and in
// which genes.  Dense counts and counts stored as their non-zeros.  The (D, B) rate and the (D, B) residuals never exist in
// HBM: the genes are taken in slabs of at most 256 MiB of fp32 residuals, laid out spot-major, which the Moran pass of
// spatial_stats.hip (moran_pass.h) reads the way it reads any (B, L) array.
//
//   m[l,n]  = exp(mean[l,n] + scale[l,n]^2 / 2)          (exp(mean) without the flag)
//   mu[d,n] = V[n] sum_l W[d,l] m[l,n]
//   kind 0, Pearson:   r = (y - mu) / sqrt(mu (1 + mu / theta))              (Poisson: theta = inf, sqrt(mu))
//   kind 1, deviance:  r = sign(y - mu) sqrt(max(d, 0)),  d the unit deviance of deviance.hip (Poisson) or nb_deviance.hip (NB)
//   I_d = sum_n z_n (1 / K) sum_k z_nbr[n,k] / sum_n z_n^2,  z = r_d - mean(r_d)
//
// The unit deviances are the cancellation-free forms of the deviance entries, restated here (deviance.hip and
// nb_deviance.hip stay as they are): y log(y / mu) as a log1p of a non-negative argument on either side of y = mu
// (dv_ylog_ratio), the compensated log1p, and the NB deviance as 2 (y A - theta B) with both logarithms log1p's of
// non-negative arguments (unit_dev).  This file is built with fp contraction off: every fused multiply-add is written out,
// so the element-wise function gives the same bits wherever it is inlined.
//
//   rs_factors_kernel   m (Lt, B); V padded to whole tiles
//   rs_tile_kernel      grid (gene blocks of 64, spot slices), 4 waves; wave w owns 16 columns of the slab and sweeps its
//                       spot slice in tiles of 64.  The tile is v_mfma_f32_16x16x4_f32 with the spots as rows (the scheme of
//                       dv_tile_kernel): a lane holds 16 spots of ONE gene, y arrives as four 16-byte loads of one row, the
//                       next tile's operands are requested before the current one is computed, y is read once.  The
//                       epilogue stores straight from the registers into slab[n * ld + column]: at a fixed spot the 16
//                       gene lanes of a wave are one 64-byte segment and the 4 waves of a workgroup are 256 consecutive
//                       bytes, so every store instruction of a wave fills four whole 64-byte segments.  The transposition
//                       is NOT staged through LDS: the direct form has no barrier in the loop and writes whole segments
//                       already; the staged form was not measured.  Columns beyond the slab's genes are written as 0.
//                       ZERO = true reads no counts (y = 0 everywhere): launch 1 of the sparse entry.  It is the same
//                       element-wise code at y = 0, which is the closed form of the zero-count residual
//                       (-sqrt(mu / (1 + mu / theta)), -sqrt(2 mu), -sqrt(2 theta log1p(mu / theta))) and gives the dense
//                       entry's bits at every element without a stored count.
//   rs_stored_kernel    launch 2 of the sparse entry: block (column, chunk group), one wave per chunk of at most 512
//                       consecutive stored entries of the column's gene row (gene_rows.h: clamped rows, checked entries).
//                       mu is formed again at each entry BY THE SAME MFMA, 64 entries at a time with the entries as rows
//                       and the gene's W in every column, so a stored entry gets the bits of the dense entry's rate; the
//                       residual overwrites the slab's element.  The factors are gathered from the (Lt, B) array of the
//                       dense pass; a transposed copy for this gather measured no faster.
//   for_ksteps          the one list of the k-step instances; launch_slab, the one launcher of a slab's residual pass (the
//                       tile kernel, or its ZERO instance and then the stored kernel), takes the kernels of either family.
//   run_slabs           the driver of every entry over a neighbour table: the checks (check_shape, check_call, check_table),
//                       make_plan (the one carve of the scratch, narrow or wide), the factors, then per slab the residual pass
//                       and the statistic its caller passes in.  No atomics, no workgroup waits on another, every sum (all of
//                       them in the Moran pass) fp64 in a fixed order: two calls agree bit for bit.
//   run_moran           gpz_residual_morans_i*: run_slabs with moran_slab_run over the narrow layout.
//   run_wide            gpz_residual_spatial_stats* and gpz_residual_autocorr_perm* (run_stats, run_perm): run_slabs over the
//                       wide layout with the wide column pass once (Geary's C and the kurtosis beside I), then every batch of
//                       permutations over the resident slab (moran_pass.h).  The slab is filled exactly as for the Moran
//                       entries.
//   Gaussian family     the Gaussian factor models (gpz_gaussian_residual*): the residual pass of residual_gaussian.h behind
//                       the same plan and the same driver (residual_slab and launch_factors dispatch on Call::gaussian); these
//                       entries always take the wide pass.  The count kernels above do not change with it.
//   entries             each builds its Call (count_call or gaussian_call, .stored(...) for data held as its non-zeros) and, for
//                       the permutation entries, its PermCall, and calls run_residuals, run_moran, run_stats or run_perm.
#include "common.h"
#include "gene_rows.h"
#include "moran_pass.h"

#include <type_traits>
#include <utility>

namespace gpz {
namespace rsd {

constexpr int MAXL = 64;          // factors
constexpr int TS = 64;            // spots per tile
constexpr int TG = 16;            // genes per wave tile
constexpr int BG = 64;            // genes per workgroup (4 waves)
constexpr int CHUNK = 512;        // sparse: stored entries of one gene row per wave
constexpr int KMAX = 32;          // neighbours
constexpr int64_t SLAB_BYTES = 256ll << 20;
constexpr int64_t SLAB_MAX = 1ll << 20;   // columns of a slab (gpz_morans_i's limit on L), whatever B
constexpr float LN2 = 0.69314718055994530942f;

typedef float f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f4 mfma4(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// log1p(x), x >= 0, compensated for the rounding of 1 + x (dv_log1p of deviance.hip)
__device__ __forceinline__ float log1p_c(float x) {
  const float u = 1.f + x;
  const float big = __builtin_fmaf(LN2, __builtin_amdgcn_logf(u), (x - (u - 1.f)) * __builtin_amdgcn_rcpf(u));
  const float small = x * __builtin_fmaf(x, __builtin_fmaf(x, 1.f / 3.f, -0.5f), 1.f);
  return x < 0x1p-12f ? small : big;
}

// the Poisson unit deviance 2 (y log(y / mu) - (y - mu)), 2 mu at y = 0 (dv_ylog_ratio and dv_term of deviance.hip)
__device__ __forceinline__ float pois_dev(float y, float mu) {
  const bool pos = y > 0.f, up = y >= mu;
  const float ys = pos ? y : 1.f;
  const float l = log1p_c(fabsf(ys - mu) * __builtin_amdgcn_rcpf(up ? mu : ys));
  const float t = pos ? (up ? y * l : -y * l) : 0.f;
  return 2.f * (t - (y - mu));
}

// the NB unit deviance 2 (y A - theta B) (unit_dev of nb_deviance.hip)
__device__ __forceinline__ float nb_dev(float y, float mu, float th) {
  const bool up = y >= mu, pos = y > 0.f;
  const float d = fabsf(y - mu), lo = up ? mu : y, hi = up ? y : mu;
  const float b = log1p_c(d * __builtin_amdgcn_rcpf(lo + th));
  const float a = log1p_c(th * d * __builtin_amdgcn_rcpf((pos ? lo : 1.f) * (hi + th)));
  const float ya = pos ? y * a : 0.f, tb = th * b;
  return 2.f * (up ? ya - tb : tb - ya);
}

__device__ __forceinline__ float residual(float y, float mu, float th, float ith, int fam, int kind) {
  const float e = y - mu;
  if (kind == 0) return e * __builtin_amdgcn_rsqf(fam ? mu * __builtin_fmaf(mu, ith, 1.f) : mu);
  const float s = __builtin_amdgcn_sqrtf(fmaxf(fam ? nb_dev(y, mu, th) : pois_dev(y, mu), 0.f));
  return e < 0.f ? -s : s;
}

struct Args {
  const float *mean, *scale, *W, *V, *theta, *y;
  const int32_t* genes;           // the scored genes (G), or null: gene g is g
  grk::GrRows rows;               // sparse counts by gene
  float *mF, *Vw;                 // (Lt, B); [Bp], V = 1 beyond B
  float* out;                     // this slab: (B, ld), column c is listed gene g0 + c
  int64_t B, D, Bp, g0, ng, ld;
  int Lt, SN, fam, kind, lognormal;
};

// the gene behind column col of the slab, -1 for a column beyond its genes (or a listed index outside [0, D)); A: Args or GArgs
template <class A>
__device__ __forceinline__ int64_t gene_of(const A& a, int64_t col) {
  if (col >= a.ng) return -1;
  const int64_t g = a.genes ? (int64_t)a.genes[a.g0 + col] : a.g0 + col;
  return g >= 0 && g < a.D ? g : -1;
}

__global__ __launch_bounds__(256) void rs_factors_kernel(Args a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (int64_t)a.Lt * a.B) {
    const float s = a.scale[i];
    a.mF[i] = expf(a.mean[i] + (a.lognormal ? 0.5f * s * s : 0.f));
  }
  if (i < a.Bp) a.Vw[i] = i < a.B ? a.V[i] : 1.f;
}

template <int KS, bool ZERO>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 4))) void rs_tile_kernel(Args a) {
  constexpr bool PFA = KS <= 8;                 // the A operand of the next tile fits in registers beside the current one
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int64_t col = ((int64_t)blockIdx.x * 4 + wave) * TG + r;   // this lane's column of the slab
  const int64_t gene = gene_of(a, col);
  const bool dok = gene >= 0, cok = col < a.ld;
  const int64_t ntiles = (a.B + TS - 1) / TS, tper = (ntiles + a.SN - 1) / a.SN;
  const int64_t t_lo = blockIdx.y * tper, t_hi = (t_lo + tper < ntiles) ? t_lo + tper : ntiles;
  const bool vec = !ZERO && (a.B & 3) == 0 && (reinterpret_cast<uintptr_t>(a.y) & 15) == 0;   // rows of y start 16-byte aligned
  const float th = (dok && a.fam) ? a.theta[gene] : 1.f, ith = 1.f / th;
  float wb[KS];                                 // B[k = factor 4 ks + q][column r]
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int l = 4 * ks + q;
    wb[ks] = (dok && l < a.Lt) ? a.W[gene * a.Lt + l] : 0.f;
  }
  const int arow = 16 * (r >> 2) + (r & 3);     // A row r of sub-tile c is spot 16 (r >> 2) + 4c + (r & 3) of the tile
  struct Tile { f4 yv[4], vv[4]; float av[4][KS]; };
  auto load_tile = [&](int64_t tt, Tile& T) __attribute__((always_inline)) {
    const int64_t n0 = tt * TS;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int64_t n = n0 + 16 * q + 4 * c;    // < Bp: the padded array covers the tile
      T.vv[c] = *reinterpret_cast<const f4*>(a.Vw + n);
      T.yv[c] = f4{0, 0, 0, 0};
      if (!ZERO && dok) {
        const float* yp = a.y + gene * a.B + n;
        if (vec && n + 3 < a.B) T.yv[c] = *reinterpret_cast<const f4*>(yp);
        else {
#pragma unroll
          for (int g = 0; g < 4; ++g) if (n + g < a.B) T.yv[c][g] = yp[g];
        }
      }
    }
  };
  auto load_a = [&](int64_t tt, Tile& T) __attribute__((always_inline)) {
    const int64_t n0 = tt * TS;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int64_t na = n0 + arow + 4 * c;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int l = 4 * ks + q;
        T.av[c][ks] = (l < a.Lt && na < a.B) ? a.mF[(int64_t)l * a.B + na] : 0.f;
      }
    }
  };
  Tile cur, nxt;
  if (t_lo < t_hi) { load_tile(t_lo, cur); if (PFA) load_a(t_lo, cur); }
  nxt = cur;
  for (int64_t tt = t_lo; tt < t_hi; ++tt) {
    const int64_t n0 = tt * TS;
    if (!PFA) load_a(tt, cur);
    if (tt + 1 < t_hi) { load_tile(tt + 1, nxt); if (PFA) load_a(tt + 1, nxt); }
    // rate tile: row 4q + g of sub-tile c is spot 16q + 4c + g, column r is this lane's gene
    f4 z[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      z[c] = f4{0, 0, 0, 0};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) z[c] = mfma4(cur.av[c][ks], wb[ks], z[c]);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int64_t n = n0 + 16 * q + 4 * c + g;
        if (cok && n < a.B) {
          const float mu = dok ? cur.vv[c][g] * z[c][g] : 1.f;
          const float res = residual(cur.yv[c][g], mu, th, ith, a.fam, a.kind);
          a.out[n * a.ld + col] = dok ? res : 0.f;
        }
      }
    cur = nxt;
  }
}

// grid (slab columns, ceil(ceil(B / CHUNK) / 4)), 4 waves: wave = one chunk of the column's gene row
template <int KS>
__global__ __launch_bounds__(256) void rs_stored_kernel(Args a) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int64_t col = blockIdx.x;
  const int64_t gene = gene_of(a, col);
  if (gene < 0) return;
  int64_t lo, hi;
  grk::gr_row(a.rows, gene, lo, hi);
  const int64_t p0 = lo + ((int64_t)blockIdx.y * 4 + wave) * CHUNK;
  if (p0 >= hi) return;                         // wave-uniform
  const int64_t p1 = p0 + CHUNK < hi ? p0 + CHUNK : hi;
  const float th = a.fam ? a.theta[gene] : 1.f, ith = 1.f / th;
  float wb[KS];                                 // B[k = factor 4 ks + q][every column]: the gene's W
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int l = 4 * ks + q;
    wb[ks] = l < a.Lt ? a.W[gene * a.Lt + l] : 0.f;
  }
  // A row i of sub-tile c is entry 16c + i of the 64; the lane's outputs are rows 4q + g, so it finishes entry
  // 16 (r >> 2) + 4q + (r & 3), taken from sub-tile r >> 2, register r & 3
  const int mine = 16 * (r >> 2) + 4 * q + (r & 3);
  for (int64_t pb = p0; pb < p1; pb += 64) {    // wave-uniform trip count: every lane reaches every MFMA
    const int64_t p = pb + lane;
    int32_t spot = -1;
    float y = 0.f;
    if (p < p1) {
      int32_t sp;
      float x;
      if (grk::gr_entry(a.rows, p, sp, x)) { spot = sp; y = x; }
    }
    f4 z[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int32_t sa = __shfl(spot, 16 * c + r);
      z[c] = f4{0, 0, 0, 0};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int l = 4 * ks + q;
        const float av = (l < a.Lt && sa >= 0) ? a.mF[(int64_t)l * a.B + sa] : 0.f;
        z[c] = mfma4(av, wb[ks], z[c]);
      }
    }
    const int32_t ms = __shfl(spot, mine);
    const float my = __shfl(y, mine);
    float zz = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int g = 0; g < 4; ++g) zz = (4 * c + g == r) ? z[c][g] : zz;
    if (ms >= 0) {
      const float mu = a.Vw[ms] * zz;
      a.out[(int64_t)ms * a.ld + col] = residual(my, mu, th, ith, a.fam, a.kind);
    }
  }
}

static int ksteps(int Lt) {                     // the instances of dv_tile_kernel: k-steps of 4 factors
  const int k = (Lt + 3) / 4;
  return k <= 10 ? k : k <= 12 ? 12 : k <= 14 ? 14 : 16;
}

// f(std::integral_constant<int, KS>) for the instance that serves Lt factors: the one place the instances are listed
template <class F, int... KS>
static int for_ksteps(int ks, F&& f, std::integer_sequence<int, KS...>) {
  int rc = -1;
  (void)((ks == KS && ((rc = f(std::integral_constant<int, KS>{})), true)) || ...);
  return rc;
}

template <class F>
static int for_ksteps(int Lt, F&& f) {
  return for_ksteps(ksteps(Lt), f, std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 16>{});
}

static int spot_slices(int64_t B, int64_t cols) {
  // enough (gene block, spot slice) workgroups to fill the device a few times over, slices of at least 8 tiles
  const int64_t GB = (cols + BG - 1) / BG;
  int64_t SN = (1024 + GB - 1) / GB;
  if (SN > (B + 511) / 512) SN = (B + 511) / 512;
  if (SN > 16) SN = 16;
  if (SN < 1) SN = 1;
  return (int)SN;
}

// The residual pass of one slab, for either family (A: Args or GArgs): the tile kernel over dense data; over stored data its
// ZERO instance and then, where anything is stored, the stored kernel over the slab's gene rows.
template <class A>
static int launch_slab(void (*tile)(A), void (*zero)(A), void (*stored)(A), const A& a, bool sparse, hipStream_t s) {
  const dim3 grid((unsigned)((a.ld + BG - 1) / BG), (unsigned)a.SN), block(256);
  hipLaunchKernelGGL(sparse ? zero : tile, grid, block, 0, s, a);
  GPZ_LAUNCH_OK();
  if (sparse && a.rows.nnz > 0) {
    const int64_t chunks = (a.B + CHUNK - 1) / CHUNK;             // a gene row holds at most B entries
    hipLaunchKernelGGL(stored, dim3((unsigned)a.ng, (unsigned)((chunks + 3) / 4)), block, 0, s, a);
    GPZ_LAUNCH_OK();
  }
  return 0;
}

}  // namespace rsd
}  // namespace gpz

#include "residual_gaussian.h"

namespace gpz {
namespace rsd {

static int count_slab(const Args& a, bool sparse, hipStream_t s) {
  return for_ksteps(a.Lt, [&](auto ks) {
    constexpr int KS = decltype(ks)::value;
    return launch_slab(rs_tile_kernel<KS, false>, rs_tile_kernel<KS, true>, rs_stored_kernel<KS>, a, sparse, s);
  });
}

constexpr int PERM_BATCH_DEFAULT = 16;          // the plan's choice where 16 tables fit; DESIGN.md section 5 says what it rests on
constexpr int64_t TABLE_BYTES = 256ll << 20;    // the tables of a batch stay within what the slab is held to

// The slabs and the scratch.  Both layouts open with the factors and the slab; the narrow one (the Moran entries) closes with
// the Moran pass's partial sums: mF, Vw, [small], slab, moran.  The wide one (the entries that need more than I) closes with
// the wide column pass's partial sums and, for the permutation entries, the batch's relabelled tables and partial sums
// (moran_pass.h): mF, Vw, slab, wide, perm.
struct Plan {
  int64_t SG, nslabs, Bp;
  int SN, KS;
  float *mF, *Vw, *slab;
  void *moran, *wide, *perm;      // narrow: moran; wide: wide, and perm with permutations
  int perm_batch;                 // 0: no permutations
  int64_t batches;
  size_t small, bytes;            // what the residual entries need; what the layout needs
};

// G: the scored genes; slab_in: the caller's slab_genes (0: the largest multiple of 64 within SLAB_BYTES).  Narrow without K;
// with K neighbours wide, for P permutations (0: the statistics alone) in batches of perm_in (0: the plan's choice)
static Plan make_plan(int64_t B, int64_t G, int Lt, int64_t slab_in, void* ws, int K = 0, int64_t P = 0, int perm_in = 0) {
  Plan p{};
  const int64_t G64 = (G + 63) / 64 * 64;
  p.SG = slab_in > 0 ? slab_in : SLAB_BYTES / (B * 4) / 64 * 64;
  if (p.SG > SLAB_MAX) p.SG = SLAB_MAX;
  if (p.SG < 64) p.SG = 64;
  if (p.SG > G64) p.SG = G64;
  p.nslabs = (G + p.SG - 1) / p.SG;
  p.Bp = (B + TS - 1) / TS * TS;
  p.SN = spot_slices(B, p.SG);
  p.KS = ksteps(Lt);
  Carver c(ws);
  p.mF = c.take<float>((size_t)Lt * B);
  p.Vw = c.take<float>((size_t)p.Bp);
  p.small = c.used();
  p.slab = c.take<float>((size_t)B * p.SG);
  if (K == 0) p.moran = c.take<char>(moran_slab_bytes(B, p.SG));
  else p.wide = c.take<char>(moran_slab_wide_bytes(B, p.SG));
  if (P > 0) {
    int64_t pb = perm_in;
    if (pb == 0) {
      const int64_t fit = TABLE_BYTES / (4 * B * K);
      pb = fit < 1 ? 1 : (fit > PERM_BATCH_DEFAULT ? PERM_BATCH_DEFAULT : fit);
    }
    if (pb > P) pb = P;
    p.perm_batch = (int)pb;
    p.batches = (P + pb - 1) / pb;
    p.perm = c.take<char>(moran_slab_perm_bytes(B, p.SG, K, p.perm_batch));
  }
  p.bytes = c.used();
  return p;
}

static int check_shape(const char* who, int64_t B, int64_t D, int64_t G, int Lt, int64_t nnz, int64_t slab_genes) {
  GPZ_REQUIRE(B >= 1 && D >= 1 && G >= 1 && nnz >= 0, "%s: bad extents (B = %lld, D = %lld, genes = %lld, nnz = %lld)", who,
              (long long)B, (long long)D, (long long)G, (long long)nnz);
  GPZ_REQUIRE(B < (1ll << 31) && D < (1ll << 31) && G < (1ll << 31) && nnz < (1ll << 31),
              "%s: spots, genes and non-zeros are indexed with 32 bits", who);
  GPZ_REQUIRE(Lt >= 1 && Lt <= MAXL, "%s: %d factors unsupported (1..%d)", who, Lt, MAXL);
  GPZ_REQUIRE(B < (1ll << 27) || nnz == 0, "%s: stored counts over %lld spots unsupported (below 2^27)", who, (long long)B);
  GPZ_REQUIRE(slab_genes >= 0 && slab_genes % 64 == 0 && slab_genes <= SLAB_MAX,
              "%s: slab_genes = %lld is not a positive multiple of 64 up to %lld (or 0: the plan's choice)", who,
              (long long)slab_genes, (long long)SLAB_MAX);
  return 0;
}

struct Call {
  const float *mean, *scale, *W, *V, *theta, *y;
  const int64_t* row_ptr; const int32_t *row_spot, *row_perm; const float* col_val;
  const int32_t* genes;
  int64_t B, D, nnz, G;
  int Lt, fam, kind, lognormal;
  bool sparse;
  const float *b, *noise_sd;      // the Gaussian family: intercept and noise standard deviation (D,) in place of V and theta,
  const double* offset;           // and the (D,) offset of expression stored as its non-zeros
  bool gaussian;                  // set by the Gaussian entries alone: fam and lognormal mean nothing there

  // the same call over data stored as its non-zeros (the sparse entries pass no y)
  Call stored(const int64_t* rp, const int32_t* rs, const int32_t* rm, const float* cv, int64_t n, const double* off = nullptr) const {
    Call c = *this;
    c.row_ptr = rp; c.row_spot = rs; c.row_perm = rm; c.col_val = cv; c.nnz = n; c.offset = off; c.sparse = true;
    return c;
  }
};

// a dense call of the count family, and of the Gaussian family
static Call count_call(const float* mean, const float* scale, const float* W, const float* V, const float* theta, const float* y,
                       const int32_t* genes, int64_t B, int64_t D, int64_t G, int Lt, int fam, int kind, int lognormal) {
  return Call{mean, scale, W, V, theta, y, nullptr, nullptr, nullptr, nullptr, genes, B, D, 0, G, Lt, fam, kind, lognormal, false,
              nullptr, nullptr, nullptr, false};
}

static Call gaussian_call(const float* mean, const float* scale, const float* W, const float* b, const float* noise_sd,
                          const float* y, const int32_t* genes, int64_t B, int64_t D, int64_t G, int Lt, int kind) {
  return Call{mean, scale, W, nullptr, nullptr, y, nullptr, nullptr, nullptr, nullptr, genes, B, D, 0, G, Lt, 0, kind, 0, false,
              b, noise_sd, nullptr, true};
}

static int check_call(const char* who, const Call& c, const void* partials) {
  if (c.gaussian) {
    GPZ_REQUIRE(c.mean && c.scale && c.W && c.b && c.noise_sd && partials, "%s: null pointer", who);
    GPZ_REQUIRE(c.sparse ? (c.row_ptr != nullptr && c.offset != nullptr) : c.y != nullptr, "%s: null pointer (expression)", who);
    GPZ_REQUIRE(!c.sparse || c.nnz == 0 || (c.row_spot && c.row_perm && c.col_val), "%s: null pointer (stored entries)", who);
    GPZ_REQUIRE(c.kind >= 0 && c.kind <= 2, "%s: kind %d unknown (0 Pearson, 1 response, 2 predictive)", who, c.kind);
  } else {
    GPZ_REQUIRE(c.mean && c.scale && c.W && c.V && partials, "%s: null pointer", who);
    GPZ_REQUIRE(c.sparse ? c.row_ptr != nullptr : c.y != nullptr, "%s: null pointer (counts)", who);
    GPZ_REQUIRE(!c.sparse || c.nnz == 0 || (c.row_spot && c.row_perm && c.col_val), "%s: null pointer (non-zeros)", who);
    GPZ_REQUIRE(c.fam == 0 || c.fam == 1, "%s: family %d unknown (0 Poisson, 1 negative binomial)", who, c.fam);
    GPZ_REQUIRE(c.kind == 0 || c.kind == 1, "%s: kind %d unknown (0 Pearson, 1 deviance)", who, c.kind);
    GPZ_REQUIRE(c.fam == 0 || c.theta, "%s: the negative binomial family needs theta", who);
  }
  GPZ_REQUIRE(c.genes || c.G == c.D, "%s: %lld genes of %lld without a list", who, (long long)c.G, (long long)c.D);
  GPZ_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 15) == 0, "%s: partials must be 16-byte aligned", who);
  return 0;
}

static void fill_args(Args& a, const Call& c, const Plan& p) {
  a.mean = c.mean; a.scale = c.scale; a.W = c.W; a.V = c.V; a.theta = c.theta; a.y = c.y; a.genes = c.genes;
  a.rows = grk::GrRows{c.row_ptr, c.row_spot, c.row_perm, c.col_val, c.B, c.D, c.nnz};
  a.mF = p.mF; a.Vw = p.Vw;
  a.B = c.B; a.D = c.D; a.Bp = p.Bp;
  a.Lt = c.Lt; a.fam = c.fam; a.kind = c.kind; a.lognormal = c.lognormal != 0;
}

static GArgs gaussian_args(const Args& a, const Call& c) {
  GArgs g;
  g.mean = c.mean; g.W = c.W; g.b = c.b; g.sd = c.noise_sd; g.y = c.y; g.offset = c.offset; g.genes = c.genes;
  g.rows = a.rows; g.s2 = a.mF; g.out = a.out;
  g.B = a.B; g.D = a.D; g.g0 = a.g0; g.ng = a.ng; g.ld = a.ld;
  g.Lt = a.Lt; g.SN = a.SN; g.kind = c.kind;
  return g;
}

// the residual pass of one slab, by family
static int residual_slab(const Args& a, const Call& c, hipStream_t s) {
  if (c.gaussian) return gs_residual_slab(gaussian_args(a, c), c.sparse, s);
  return count_slab(a, c.sparse, s);
}

static int launch_factors(const Args& a, const Call& c, hipStream_t s) {
  if (c.gaussian) {                             // the means are read where they are; scale^2 for the predictive kind alone
    if (c.kind != 2) return 0;
    const int64_t n = (int64_t)a.Lt * a.B;
    hipLaunchKernelGGL(gs_factors_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, c.scale, a.mF, n);
    GPZ_LAUNCH_OK();
    return 0;
  }
  const int64_t tot = (int64_t)a.Lt * a.B > a.Bp ? (int64_t)a.Lt * a.B : a.Bp;
  hipLaunchKernelGGL(rs_factors_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, a);
  GPZ_LAUNCH_OK();
  return 0;
}

// residuals of the listed genes into out (B, G)
static int run_residuals(const char* who, const Call& c, float* out, void* partials, size_t partials_bytes, void* stream) {
  if (int rc = check_shape(who, c.B, c.D, c.G, c.Lt, c.nnz, 0)) return rc;
  if (int rc = check_call(who, c, partials)) return rc;
  GPZ_REQUIRE(out, "%s: null pointer", who);
  const Plan p = make_plan(c.B, c.G, c.Lt, 64, partials);
  GPZ_REQUIRE(partials_bytes >= p.small, "%s: partials too small (%zu bytes, %zu needed)", who, partials_bytes, p.small);
  hipStream_t s = static_cast<hipStream_t>(stream);
  Args a;
  fill_args(a, c, p);
  a.out = out; a.g0 = 0; a.ng = c.G; a.ld = c.G; a.SN = spot_slices(c.B, c.G);
  if (int rc = launch_factors(a, c, s)) return rc;
  return residual_slab(a, c, s);
}

static int check_table(const char* who, int64_t B, int K) {
  GPZ_REQUIRE(K >= 1 && K <= KMAX && B > K, "%s: K = %d neighbours of %lld spots unsupported (1 <= K <= %d, K < B)", who, K,
              (long long)B, KMAX);
  return 0;
}

// The entries over a neighbour table: the checks, the plan (wide: see make_plan; P permutations in batches of perm_batch),
// the factors, then per slab the residual pass and stat(a, p, s), the statistic of the slab that a describes.  outs: the
// entry's output pointers are all there.
template <class Stat>
static int run_slabs(const char* who, const Call& c, const int64_t* nbr, int K, int64_t slab_genes, bool wide, int64_t P,
                     int perm_batch, bool outs, int32_t* info, void* partials, size_t partials_bytes, void* stream, Stat stat) {
  if (int rc = check_shape(who, c.B, c.D, c.G, c.Lt, c.nnz, slab_genes)) return rc;
  if (int rc = check_call(who, c, partials)) return rc;
  GPZ_REQUIRE(nbr && outs && info, "%s: null pointer", who);
  if (int rc = check_table(who, c.B, K)) return rc;
  const Plan p = make_plan(c.B, c.G, c.Lt, slab_genes, partials, wide ? K : 0, P, perm_batch);
  GPZ_REQUIRE(partials_bytes >= p.bytes, "%s: partials too small (%zu bytes, %zu needed)", who, partials_bytes, p.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  GPZ_HIP_OK(hipMemsetAsync(info, 0, sizeof(int32_t), s));
  Args a;
  fill_args(a, c, p);
  a.out = p.slab; a.SN = p.SN;
  if (int rc = launch_factors(a, c, s)) return rc;
  for (int64_t sl = 0; sl < p.nslabs; ++sl) {
    a.g0 = sl * p.SG;
    a.ng = c.G - a.g0 < p.SG ? c.G - a.g0 : p.SG;
    a.ld = (a.ng + 63) / 64 * 64;               // the last slab is as wide as its genes, rounded up to a block
    if (int rc = residual_slab(a, c, s)) return rc;
    if (int rc = stat(a, p, s)) return rc;
  }
  return 0;
}

static int run_moran(const char* who, const Call& c, const int64_t* nbr, int K, int64_t slab_genes, double* I, double* res_mean,
                     double* res_var, int32_t* info, void* partials, size_t partials_bytes, void* stream) {
  return run_slabs(who, c, nbr, K, slab_genes, false, 0, 0, I && res_mean && res_var, info, partials, partials_bytes, stream,
                   [&](const Args& a, const Plan& p, hipStream_t s) {
                     return moran_slab_run(p.slab, c.B, a.ng, a.ld, nbr, K, I + a.g0, res_mean + a.g0, res_var + a.g0, info,
                                           p.moran, s);
                   });
}

// ---- the wide statistics and the permutation null -------------------------------------------------------------------

static int check_perm(const char* who, int64_t P, int stat, int perm_batch) {
  GPZ_REQUIRE(P >= 1 && P < (1ll << 31), "%s: P = %lld permutations unsupported (1 <= P < 2^31)", who, (long long)P);
  GPZ_REQUIRE(stat == 0 || stat == 1, "%s: stat %d unknown (0 Moran's I, 1 Geary's C)", who, stat);
  GPZ_REQUIRE(perm_batch >= 0 && perm_batch <= SLAB_PERM_BATCH_MAX, "%s: perm_batch = %d unsupported (0 = chosen here, at most %d)",
              who, perm_batch, SLAB_PERM_BATCH_MAX);
  return 0;
}

struct PermCall {                 // perms == nullptr: the statistics alone
  const int32_t* perms;
  int64_t P;
  int stat, perm_batch;
  double *value, *sims;
  int32_t *n_ge, *n_le;
  double *sim_mean, *sim_m2;
};

// Per slab: the residual pass once, the wide column pass once, then every batch of permutations.  Without permutations the
// five statistics go to I, C, res_mean, res_var, kurtosis; with them the observed statistic goes to pc.value and the other
// of I and C into the scratch.
static int run_wide(const char* who, const Call& c, const int64_t* nbr, int K, int64_t slab_genes, double* I, double* C,
                    double* res_mean, double* res_var, double* kurtosis, const PermCall& pc, int32_t* info, void* partials,
                    size_t partials_bytes, void* stream) {
  const bool permute = pc.perms != nullptr;
  const bool outs = (I || C) && (permute || (I && C)) && res_mean && res_var && kurtosis;
  return run_slabs(
      who, c, nbr, K, slab_genes, true, permute ? pc.P : 0, pc.perm_batch, outs, info, partials, partials_bytes, stream,
      [&](const Args& a, const Plan& p, hipStream_t s) {
        if (int rc = moran_slab_wide_run(p.slab, c.B, a.ng, a.ld, nbr, K, I ? I + a.g0 : nullptr, C ? C + a.g0 : nullptr,
                                         res_mean + a.g0, res_var + a.g0, kurtosis + a.g0, info, p.wide, s))
          return rc;
        if (!permute) return 0;
        const SlabPermOut o{pc.n_ge + a.g0, pc.n_le + a.g0, pc.sim_mean + a.g0, pc.sim_m2 + a.g0,
                            pc.sims ? pc.sims + a.g0 * pc.P : nullptr, pc.P, info};
        GPZ_HIP_OK(hipMemsetAsync(o.n_ge, 0, size_t(a.ng) * sizeof(int32_t), s));      // the batches accumulate into these
        GPZ_HIP_OK(hipMemsetAsync(o.n_le, 0, size_t(a.ng) * sizeof(int32_t), s));
        GPZ_HIP_OK(hipMemsetAsync(o.sim_mean, 0, size_t(a.ng) * sizeof(double), s));
        GPZ_HIP_OK(hipMemsetAsync(o.sim_m2, 0, size_t(a.ng) * sizeof(double), s));
        return moran_slab_perm_run(p.slab, c.B, a.ng, a.ld, nbr, K, pc.stat, pc.perms, pc.P, p.perm_batch, res_mean + a.g0, p.wide,
                                   o, p.perm, s);
      });
}

static int run_stats(const char* who, const Call& c, const int64_t* nbr, int K, int64_t slab_genes, double* I, double* C,
                     double* res_mean, double* res_var, double* kurtosis, int32_t* info, void* partials, size_t partials_bytes,
                     void* stream) {
  return run_wide(who, c, nbr, K, slab_genes, I, C, res_mean, res_var, kurtosis, PermCall{}, info, partials, partials_bytes, stream);
}

// value is the observed I or C; the wide pass does not write the other of the two
static int run_perm(const char* who, const Call& c, const int64_t* nbr, int K, int64_t slab_genes, const PermCall& pc,
                    double* res_mean, double* res_var, double* kurtosis, int32_t* info, void* partials, size_t partials_bytes,
                    void* stream) {
  GPZ_REQUIRE(pc.perms && pc.value && pc.n_ge && pc.n_le && pc.sim_mean && pc.sim_m2, "%s: null pointer", who);
  if (int rc = check_perm(who, pc.P, pc.stat, pc.perm_batch)) return rc;
  return run_wide(who, c, nbr, K, slab_genes, pc.stat == 0 ? pc.value : nullptr, pc.stat == 0 ? nullptr : pc.value, res_mean,
                  res_var, kurtosis, pc, info, partials, partials_bytes, stream);
}

// What the plan queries of the entries over a table answer; K >= 1, P = 0: the scratch of the stats entries, no permutation arrays
static int wide_plan(const char* who, int64_t B, int64_t D, int Lt, int K, int64_t P, int64_t nnz, int64_t slab_genes_wanted,
                     int perm_batch_wanted, int64_t* slab_genes, int64_t* n_slabs, int32_t* spot_slices, int32_t* factors_padded,
                     int32_t* perm_batch, int64_t* batches, int64_t* partials_bytes) {
  if (int rc = check_shape(who, B, D, D, Lt, nnz, slab_genes_wanted)) return rc;
  if (int rc = check_table(who, B, K)) return rc;
  if (P != 0)
    if (int rc = check_perm(who, P, 0, perm_batch_wanted)) return rc;
  const Plan p = make_plan(B, D, Lt, slab_genes_wanted, nullptr, K, P, perm_batch_wanted);
  if (slab_genes) *slab_genes = p.SG;
  if (n_slabs) *n_slabs = p.nslabs;
  if (spot_slices) *spot_slices = p.SN;
  if (factors_padded) *factors_padded = 4 * p.KS;
  if (perm_batch) *perm_batch = p.perm_batch;
  if (batches) *batches = p.batches;
  if (partials_bytes) *partials_bytes = (int64_t)p.bytes;
  return 0;
}

}  // namespace rsd
}  // namespace gpz

using namespace gpz;

extern "C" int gpz_residual_morans_i_plan(int64_t B, int64_t D, int32_t Lt, int64_t nnz, int64_t slab_genes_wanted,
                                          int64_t* slab_genes, int64_t* n_slabs, int32_t* spots_per_tile,
                                          int32_t* genes_per_block, int32_t* spot_slices, int32_t* gene_chunk,
                                          int32_t* factors_padded, int64_t* partials_bytes) {
  if (int rc = rsd::check_shape("gpz_residual_morans_i_plan", B, D, D, Lt, nnz, slab_genes_wanted)) return rc;
  const rsd::Plan p = rsd::make_plan(B, D, Lt, slab_genes_wanted, nullptr);
  if (slab_genes) *slab_genes = p.SG;
  if (n_slabs) *n_slabs = p.nslabs;
  if (spots_per_tile) *spots_per_tile = rsd::TS;
  if (genes_per_block) *genes_per_block = rsd::BG;
  if (spot_slices) *spot_slices = p.SN;
  if (gene_chunk) *gene_chunk = rsd::CHUNK;
  if (factors_padded) *factors_padded = 4 * p.KS;
  if (partials_bytes) *partials_bytes = (int64_t)p.bytes;
  return 0;
}

extern "C" int gpz_count_residuals(const float* mean, const float* scale, const float* W, const float* V, const float* theta,
                                   const float* y, const int32_t* genes, int64_t B, int64_t D, int64_t G, int32_t Lt,
                                   int32_t family, int32_t kind, int32_t lognormal_mean, float* out, void* partials,
                                   size_t partials_bytes, void* stream) {
  const rsd::Call c = rsd::count_call(mean, scale, W, V, theta, y, genes, B, D, G, Lt, family, kind, lognormal_mean);
  return rsd::run_residuals("gpz_count_residuals", c, out, partials, partials_bytes, stream);
}

extern "C" int gpz_count_residuals_sparse(const float* mean, const float* scale, const float* W, const float* V,
                                          const float* theta, const int64_t* row_ptr, const int32_t* row_spot,
                                          const int32_t* row_perm, const float* col_val, const int32_t* genes, int64_t B,
                                          int64_t D, int64_t nnz, int64_t G, int32_t Lt, int32_t family, int32_t kind,
                                          int32_t lognormal_mean, float* out, void* partials, size_t partials_bytes,
                                          void* stream) {
  const rsd::Call c = rsd::count_call(mean, scale, W, V, theta, nullptr, genes, B, D, G, Lt, family, kind, lognormal_mean)
                          .stored(row_ptr, row_spot, row_perm, col_val, nnz);
  return rsd::run_residuals("gpz_count_residuals_sparse", c, out, partials, partials_bytes, stream);
}

extern "C" int gpz_residual_morans_i(const float* mean, const float* scale, const float* W, const float* V, const float* theta,
                                     const float* y, const int32_t* genes, const int64_t* nbr, int64_t B, int64_t D, int64_t G,
                                     int32_t Lt, int32_t K, int32_t family, int32_t kind, int32_t lognormal_mean,
                                     int64_t slab_genes, double* I, double* res_mean, double* res_var, int32_t* info,
                                     void* partials, size_t partials_bytes, void* stream) {
  const rsd::Call c = rsd::count_call(mean, scale, W, V, theta, y, genes, B, D, G, Lt, family, kind, lognormal_mean);
  return rsd::run_moran("gpz_residual_morans_i", c, nbr, K, slab_genes, I, res_mean, res_var, info, partials, partials_bytes,
                        stream);
}

extern "C" int gpz_residual_morans_i_sparse(const float* mean, const float* scale, const float* W, const float* V,
                                            const float* theta, const int64_t* row_ptr, const int32_t* row_spot,
                                            const int32_t* row_perm, const float* col_val, const int32_t* genes,
                                            const int64_t* nbr, int64_t B, int64_t D, int64_t nnz, int64_t G, int32_t Lt,
                                            int32_t K, int32_t family, int32_t kind, int32_t lognormal_mean, int64_t slab_genes,
                                            double* I, double* res_mean, double* res_var, int32_t* info, void* partials,
                                            size_t partials_bytes, void* stream) {
  const rsd::Call c = rsd::count_call(mean, scale, W, V, theta, nullptr, genes, B, D, G, Lt, family, kind, lognormal_mean)
                          .stored(row_ptr, row_spot, row_perm, col_val, nnz);
  return rsd::run_moran("gpz_residual_morans_i_sparse", c, nbr, K, slab_genes, I, res_mean, res_var, info, partials,
                        partials_bytes, stream);
}

extern "C" int gpz_residual_autocorr_perm_plan(int64_t B, int64_t D, int32_t Lt, int32_t K, int64_t P, int64_t nnz,
                                               int64_t slab_genes_wanted, int32_t perm_batch_wanted, int64_t* slab_genes,
                                               int64_t* n_slabs, int32_t* perm_batch, int64_t* batches, int64_t* partials_bytes) {
  return rsd::wide_plan("gpz_residual_autocorr_perm_plan", B, D, Lt, K, P, nnz, slab_genes_wanted, perm_batch_wanted, slab_genes,
                        n_slabs, nullptr, nullptr, perm_batch, batches, partials_bytes);
}

extern "C" int gpz_residual_spatial_stats(const float* mean, const float* scale, const float* W, const float* V, const float* theta,
                                          const float* y, const int32_t* genes, const int64_t* nbr, int64_t B, int64_t D, int64_t G,
                                          int32_t Lt, int32_t K, int32_t family, int32_t kind, int32_t lognormal_mean,
                                          int64_t slab_genes, double* I, double* C, double* res_mean, double* res_var,
                                          double* kurtosis, int32_t* info, void* partials, size_t partials_bytes, void* stream) {
  const rsd::Call c = rsd::count_call(mean, scale, W, V, theta, y, genes, B, D, G, Lt, family, kind, lognormal_mean);
  return rsd::run_stats("gpz_residual_spatial_stats", c, nbr, K, slab_genes, I, C, res_mean, res_var, kurtosis, info, partials,
                        partials_bytes, stream);
}

extern "C" int gpz_residual_spatial_stats_sparse(const float* mean, const float* scale, const float* W, const float* V,
                                                 const float* theta, const int64_t* row_ptr, const int32_t* row_spot,
                                                 const int32_t* row_perm, const float* col_val, const int32_t* genes,
                                                 const int64_t* nbr, int64_t B, int64_t D, int64_t nnz, int64_t G, int32_t Lt,
                                                 int32_t K, int32_t family, int32_t kind, int32_t lognormal_mean,
                                                 int64_t slab_genes, double* I, double* C, double* res_mean, double* res_var,
                                                 double* kurtosis, int32_t* info, void* partials, size_t partials_bytes,
                                                 void* stream) {
  const rsd::Call c = rsd::count_call(mean, scale, W, V, theta, nullptr, genes, B, D, G, Lt, family, kind, lognormal_mean)
                          .stored(row_ptr, row_spot, row_perm, col_val, nnz);
  return rsd::run_stats("gpz_residual_spatial_stats_sparse", c, nbr, K, slab_genes, I, C, res_mean, res_var, kurtosis, info,
                        partials, partials_bytes, stream);
}

extern "C" int gpz_residual_autocorr_perm(const float* mean, const float* scale, const float* W, const float* V, const float* theta,
                                          const float* y, const int32_t* genes, const int64_t* nbr, const int32_t* perms, int64_t B,
                                          int64_t D, int64_t G, int32_t Lt, int32_t K, int32_t family, int32_t kind,
                                          int32_t lognormal_mean, int64_t slab_genes, int64_t P, int32_t stat, int32_t perm_batch,
                                          double* value, int32_t* n_ge, int32_t* n_le, double* sim_mean, double* sim_m2,
                                          double* sims, double* res_mean, double* res_var, double* kurtosis, int32_t* info,
                                          void* partials, size_t partials_bytes, void* stream) {
  const rsd::Call c = rsd::count_call(mean, scale, W, V, theta, y, genes, B, D, G, Lt, family, kind, lognormal_mean);
  const rsd::PermCall pc{perms, P, stat, perm_batch, value, sims, n_ge, n_le, sim_mean, sim_m2};
  return rsd::run_perm("gpz_residual_autocorr_perm", c, nbr, K, slab_genes, pc, res_mean, res_var, kurtosis, info, partials,
                       partials_bytes, stream);
}

extern "C" int gpz_residual_autocorr_perm_sparse(const float* mean, const float* scale, const float* W, const float* V,
                                                 const float* theta, const int64_t* row_ptr, const int32_t* row_spot,
                                                 const int32_t* row_perm, const float* col_val, const int32_t* genes,
                                                 const int64_t* nbr, const int32_t* perms, int64_t B, int64_t D, int64_t nnz,
                                                 int64_t G, int32_t Lt, int32_t K, int32_t family, int32_t kind,
                                                 int32_t lognormal_mean, int64_t slab_genes, int64_t P, int32_t stat,
                                                 int32_t perm_batch, double* value, int32_t* n_ge, int32_t* n_le, double* sim_mean,
                                                 double* sim_m2, double* sims, double* res_mean, double* res_var, double* kurtosis,
                                                 int32_t* info, void* partials, size_t partials_bytes, void* stream) {
  const rsd::Call c = rsd::count_call(mean, scale, W, V, theta, nullptr, genes, B, D, G, Lt, family, kind, lognormal_mean)
                          .stored(row_ptr, row_spot, row_perm, col_val, nnz);
  const rsd::PermCall pc{perms, P, stat, perm_batch, value, sims, n_ge, n_le, sim_mean, sim_m2};
  return rsd::run_perm("gpz_residual_autocorr_perm_sparse", c, nbr, K, slab_genes, pc, res_mean, res_var, kurtosis, info, partials,
                       partials_bytes, stream);
}

// ---- the Gaussian factor models ---------------------------------------------------------------------------------------
// K = 0 (with P = 0): what gpz_gaussian_residuals* need, the factor scratch alone.

extern "C" int gpz_gaussian_residual_plan(int64_t B, int64_t D, int32_t Lt, int32_t K, int64_t P, int64_t nnz,
                                          int64_t slab_genes_wanted, int32_t perm_batch_wanted, int64_t* slab_genes,
                                          int64_t* n_slabs, int32_t* spot_slices, int32_t* factors_padded, int32_t* perm_batch,
                                          int64_t* batches, int64_t* partials_bytes) {
  const char* who = "gpz_gaussian_residual_plan";
  if (K != 0)
    return rsd::wide_plan(who, B, D, Lt, K, P, nnz, slab_genes_wanted, perm_batch_wanted, slab_genes, n_slabs, spot_slices,
                          factors_padded, perm_batch, batches, partials_bytes);
  if (int rc = rsd::check_shape(who, B, D, D, Lt, nnz, slab_genes_wanted)) return rc;
  GPZ_REQUIRE(P == 0, "%s: P = %lld permutations without a neighbour table (K = 0)", who, (long long)P);
  const rsd::Plan p = rsd::make_plan(B, D, Lt, 64, nullptr);
  if (slab_genes) *slab_genes = p.SG;
  if (n_slabs) *n_slabs = p.nslabs;
  if (spot_slices) *spot_slices = rsd::spot_slices(B, D);
  if (factors_padded) *factors_padded = 4 * p.KS;
  if (perm_batch) *perm_batch = 0;
  if (batches) *batches = 0;
  if (partials_bytes) *partials_bytes = (int64_t)p.small;
  return 0;
}

extern "C" int gpz_gaussian_residuals(const float* mean, const float* scale, const float* W, const float* b, const float* noise_sd,
                                      const float* y, const int32_t* genes, int64_t B, int64_t D, int64_t G, int32_t Lt,
                                      int32_t kind, float* out, void* partials, size_t partials_bytes, void* stream) {
  const rsd::Call c = rsd::gaussian_call(mean, scale, W, b, noise_sd, y, genes, B, D, G, Lt, kind);
  return rsd::run_residuals("gpz_gaussian_residuals", c, out, partials, partials_bytes, stream);
}

extern "C" int gpz_gaussian_residuals_sparse(const float* mean, const float* scale, const float* W, const float* b,
                                             const float* noise_sd, const double* offset, const int64_t* row_ptr,
                                             const int32_t* row_spot, const int32_t* row_perm, const float* col_val,
                                             const int32_t* genes, int64_t B, int64_t D, int64_t nnz, int64_t G, int32_t Lt,
                                             int32_t kind, float* out, void* partials, size_t partials_bytes, void* stream) {
  const rsd::Call c = rsd::gaussian_call(mean, scale, W, b, noise_sd, nullptr, genes, B, D, G, Lt, kind)
                          .stored(row_ptr, row_spot, row_perm, col_val, nnz, offset);
  return rsd::run_residuals("gpz_gaussian_residuals_sparse", c, out, partials, partials_bytes, stream);
}

extern "C" int gpz_gaussian_residual_stats(const float* mean, const float* scale, const float* W, const float* b,
                                           const float* noise_sd, const float* y, const int32_t* genes, const int64_t* nbr,
                                           int64_t B, int64_t D, int64_t G, int32_t Lt, int32_t K, int32_t kind, int64_t slab_genes,
                                           double* I, double* C, double* res_mean, double* res_var, double* kurtosis, int32_t* info,
                                           void* partials, size_t partials_bytes, void* stream) {
  const rsd::Call c = rsd::gaussian_call(mean, scale, W, b, noise_sd, y, genes, B, D, G, Lt, kind);
  return rsd::run_stats("gpz_gaussian_residual_stats", c, nbr, K, slab_genes, I, C, res_mean, res_var, kurtosis, info, partials,
                        partials_bytes, stream);
}

extern "C" int gpz_gaussian_residual_stats_sparse(const float* mean, const float* scale, const float* W, const float* b,
                                                  const float* noise_sd, const double* offset, const int64_t* row_ptr,
                                                  const int32_t* row_spot, const int32_t* row_perm, const float* col_val,
                                                  const int32_t* genes, const int64_t* nbr, int64_t B, int64_t D, int64_t nnz,
                                                  int64_t G, int32_t Lt, int32_t K, int32_t kind, int64_t slab_genes, double* I,
                                                  double* C, double* res_mean, double* res_var, double* kurtosis, int32_t* info,
                                                  void* partials, size_t partials_bytes, void* stream) {
  const rsd::Call c = rsd::gaussian_call(mean, scale, W, b, noise_sd, nullptr, genes, B, D, G, Lt, kind)
                          .stored(row_ptr, row_spot, row_perm, col_val, nnz, offset);
  return rsd::run_stats("gpz_gaussian_residual_stats_sparse", c, nbr, K, slab_genes, I, C, res_mean, res_var, kurtosis, info,
                        partials, partials_bytes, stream);
}

extern "C" int gpz_gaussian_residual_perm(const float* mean, const float* scale, const float* W, const float* b,
                                          const float* noise_sd, const float* y, const int32_t* genes, const int64_t* nbr,
                                          const int32_t* perms, int64_t B, int64_t D, int64_t G, int32_t Lt, int32_t K, int32_t kind,
                                          int64_t slab_genes, int64_t P, int32_t stat, int32_t perm_batch, double* value,
                                          int32_t* n_ge, int32_t* n_le, double* sim_mean, double* sim_m2, double* sims,
                                          double* res_mean, double* res_var, double* kurtosis, int32_t* info, void* partials,
                                          size_t partials_bytes, void* stream) {
  const rsd::Call c = rsd::gaussian_call(mean, scale, W, b, noise_sd, y, genes, B, D, G, Lt, kind);
  const rsd::PermCall pc{perms, P, stat, perm_batch, value, sims, n_ge, n_le, sim_mean, sim_m2};
  return rsd::run_perm("gpz_gaussian_residual_perm", c, nbr, K, slab_genes, pc, res_mean, res_var, kurtosis, info, partials,
                       partials_bytes, stream);
}

extern "C" int gpz_gaussian_residual_perm_sparse(const float* mean, const float* scale, const float* W, const float* b,
                                                 const float* noise_sd, const double* offset, const int64_t* row_ptr,
                                                 const int32_t* row_spot, const int32_t* row_perm, const float* col_val,
                                                 const int32_t* genes, const int64_t* nbr, const int32_t* perms, int64_t B,
                                                 int64_t D, int64_t nnz, int64_t G, int32_t Lt, int32_t K, int32_t kind,
                                                 int64_t slab_genes, int64_t P, int32_t stat, int32_t perm_batch, double* value,
                                                 int32_t* n_ge, int32_t* n_le, double* sim_mean, double* sim_m2, double* sims,
                                                 double* res_mean, double* res_var, double* kurtosis, int32_t* info,
                                                 void* partials, size_t partials_bytes, void* stream) {
  const rsd::Call c = rsd::gaussian_call(mean, scale, W, b, noise_sd, nullptr, genes, B, D, G, Lt, kind)
                          .stored(row_ptr, row_spot, row_perm, col_val, nnz, offset);
  const rsd::PermCall pc{perms, P, stat, perm_batch, value, sims, n_ge, n_le, sim_mean, sim_m2};
  return rsd::run_perm("gpz_gaussian_residual_perm_sparse", c, nbr, K, slab_genes, pc, res_mean, res_var, kurtosis, info, partials,
                       partials_bytes, stream);
}
