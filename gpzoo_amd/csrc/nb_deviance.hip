// nb_deviance.hip -- held-out scoring of counts under a negative-binomial likelihood with one inverse dispersion theta[d]
// per gene and the predictive mean rate of a fitted NSF factor model: the NB deviance with the null model's beside it, the
// NB log density, and the Poisson log density of the same rate, per gene, per spot and in total; dense counts and counts
// stored as their non-zeros.  The NB sibling of deviance.hip; the (D, N) rate never exists in HBM.
//
//   m[l,n]   = exp(mean[l,n] + scale[l,n]^2 / 2)         (exp(mean) without the flag)
//   mu[d,n]  = V[n] sum_l W[d,l] m[l,n]
//   dev[d,n] = 2 [ y log(y / mu) - (y + theta) log1p((y - mu) / (mu + theta)) ]      (the first term exactly 0 at y = 0)
//   ll[d,n]  = lgamma(y + theta) - lgamma(theta) - lgamma(y + 1) + y log(mu / (mu + theta)) - theta log1p(mu / theta)
//   pll[d,n] = y log mu - mu - lgamma(y + 1)  =  -(y log(y / mu) - y + mu) - [lgamma(y + 1) - (y log y - y)]
//   null model mu0[d,n] = V[n] r_d, r_d = sum_n y[d,n] / sum_n V[n] (the Poisson null's rate, with the gene's own theta):
//   the same dev with mu0 in place of mu; exactly 0 for a gene without counts.
//
// The deviance is evaluated as 2 (y A - theta B), A = log(y (mu + theta) / (mu (y + theta))), B = log((y + theta) / (mu + theta)),
// each a log1p with a non-negative argument on either side of y = mu (unit_dev), so no argument approaches -1, y = 0 gives
// 2 theta log1p(mu / theta) by the same code, and neither a small theta nor a large count next to its rate costs digits.
// log1p is the compensated one of nb.hip: u = 1 + x, log1p(x) = log(u) + (x - (u - 1)) / u.  The Poisson log density is
// formed as minus half the Poisson unit deviance, whose y log(y / mu) = y (A + B) comes with the NB deviance, minus
// Stirling's remainder of lgamma(y + 1), a term in y alone.
//
// The lgamma terms (and Stirling's remainder) depend on y and theta only.  For integer counts below 16 they come from a per-gene table in fp64
// (lgamma(y + theta) - lgamma(theta) = sum_{k<y} log(theta + k), the recurrence of nb.hip); every other count takes the fp64
// lgamma.  They are summed in fp64, per gene and per spot, by a pass of their own that also forms sum_n y -- the null
// model's rate has to be known before the element-wise pass, so y is read twice.
//
// Dense (gpz_nb_deviance), fp32 element-wise work, fp64 sums, no atomics, every sum in a fixed order:
//   nd_factors_kernel   m (Lt, N); V padded to whole tiles
//   nd_vsum_kernel      sum_n V[n]
//   nd_table_kernel     T[d][y] = lgamma(y + theta) - lgamma(theta) - lgamma(y + 1), y < 16; lgamma(theta[d]); Stirling's
//                       remainder lgamma(y + 1) - (y log y - y), y < 16
//   nd_const_kernel     grid (ceil(D / 64), spot slices): sum y and the lgamma sums per gene and slice, per spot and gene block
//   nd_rate_kernel      per gene: the slices in order, r_d
//   nd_tile_kernel      the tile scheme of dv_tile_kernel (16 genes x 64 spots per wave on v_mfma_f32_16x16x4_f32, spots as
//                       rows, next tile's operands prefetched): deviance, null deviance, the rate-dependent parts of both
//                       log densities and sum mu per gene; deviance and log density per spot through the halving exchange
//                       into two slabs per 64-gene block
//   nd_finish_kernel, nd_spot_sum_kernel, nd_total_kernel
//
// Sparse (gpz_nb_deviance_sparse).  With z(mu) = theta log1p(mu / theta):
//   dev = 2 z(mu) over ALL (d, n) + sum_stored 2 [ y log(y (mu + theta) / (mu (y + theta))) - theta log1p(y / theta) ]
//   ll  = - z(mu) over ALL (d, n) + sum_stored [ y log(mu / (mu + theta)) + lgamma terms ]
//   pll = - mu    over ALL (d, n) + sum_stored [ y - y log(y / mu) - Stirling's remainder ]
// One dense zero pass (nd_tile_kernel without counts) gives sum z, sum mu and the null's sum z(V r_d) per gene and sum z
// per spot; r_d comes first from a pass over the gene rows' stored entries (nds_const_kernel, O(nnz)).  The corrections
// use the work split of deviance.hip's sparse half: one wave per batch spot, one wave per chunk of at most 512
// consecutive non-zeros of a gene row.  The workspace holds nothing of D x B or nnz elements.
#include "common.h"
#include "mmops.h"
#include "sparse_rows.h"

namespace gpz {
namespace nbd {

constexpr int MAXL = 64;          // factors
constexpr int TS = 64;            // spots per tile
constexpr int TG = 16;            // genes per wave tile
constexpr int BG = 64;            // genes per workgroup (4 waves): one per-spot slab each
constexpr int CHUNK = 512;        // sparse: non-zeros of one gene row per wave
constexpr int TAB = 16;           // integer counts below this take the lgamma terms from the table
constexpr int TROW = TAB + 2;     // a gene's table row: T[0 .. 15], lgamma(theta), theta
constexpr int CQ = 3;             // per-gene sums of the const pass: y and const_terms' cl and st
constexpr int GQ = 5;             // per-gene sums of the tile pass: deviance, mu, null deviance, ll and pll rate parts
constexpr int ZQ = 3;             // per-gene sums of the zero pass: z(mu), mu, z(mu0)
constexpr int NSCAL = 6;          // total, sum y, sum mu, null total, loglik, poisson loglik
constexpr float LN2 = 0.69314718055994530942f;

typedef float f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f4 mfma4(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// log1p(x), x >= 0, compensated for the rounding of 1 + x (see the head of nb.hip); below 2^-12 the series
// x - x^2 / 2 + x^3 / 3 (its first omitted term is below 4e-12 x), so that nothing rests on the logarithm next to 1
__device__ __forceinline__ float log1p_c(float x) {
  const float u = 1.f + x;
  const float big = __builtin_fmaf(LN2, __builtin_amdgcn_logf(u), (x - (u - 1.f)) * __builtin_amdgcn_rcpf(u));
  const float small = x * __builtin_fmaf(x, __builtin_fmaf(x, 1.f / 3.f, -0.5f), 1.f);
  return x < 0x1p-12f ? small : big;
}

// The unit NB deviance and y log(y / mu).  With lo = min(y, mu), hi = max(y, mu), d = hi - lo:
//   A = log1p(theta d / (lo (hi + theta)))  = |log(y (mu + theta) / (mu (y + theta)))|      (not formed at y = 0)
//   B = log1p(d / (lo + theta))             = |log((y + theta) / (mu + theta))|
//   dev = 2 (y A - theta B) for y >= mu, 2 (theta B - y A) for y < mu;   y log(y / mu) = +- y (A + B).
// This is dev = 2 [y log(y / mu) - (y + theta) log((y + theta) / (mu + theta))] with the two terms in y taken together: apart,
// they agree to theta / y of their size where theta << mu (theta = 1e-2 at counts of 1e4: six digits lost), and
// y log(y / mu) from two logarithms loses a large count next to its rate (see dv_ylog_ratio of deviance.hip).  Every log1p
// has a non-negative argument; what is left to cancel, y A against theta B, is the deviance being of second order in d / mu.
struct Unit { float dev, yl; };
__device__ __forceinline__ Unit unit_dev(float y, float mu, float th) {
  const bool up = y >= mu, pos = y > 0.f;
  const float d = fabsf(y - mu), lo = up ? mu : y, hi = up ? y : mu;
  const float b = log1p_c(d * __builtin_amdgcn_rcpf(lo + th));
  const float a = log1p_c(th * d * __builtin_amdgcn_rcpf((pos ? lo : 1.f) * (hi + th)));
  const float ya = pos ? y * a : 0.f, tb = th * b;
  return Unit{2.f * (up ? ya - tb : tb - ya), pos ? (up ? y * (a + b) : -y * (a + b)) : 0.f};
}

// a stored count's corrections to the zero parts 2 z(mu), -z(mu), -mu: the deviance's, 2 (+- y A - theta log1p(y / theta)) with
// the A of unit_dev; the log density's (the lgamma terms apart); and the Poisson log density's, y - y log(y / mu) -- with
// the zero part -(y log(y / mu) - y + mu), half the Poisson unit deviance; the terms in y alone are const_terms' st
struct Corr { float dev, ll, pl; };
__device__ __forceinline__ Corr stored_corr(float y, float mu, float th, float ith, float l2th) {
  const float l2mu = __builtin_amdgcn_logf(mu);
  const float lm = log1p_c(mu * ith), ly = log1p_c(y * ith);
  const bool up = y >= mu;
  const float d = fabsf(y - mu), lo = up ? mu : y, hi = up ? y : mu;
  const float ya = y * log1p_c(th * d * __builtin_amdgcn_rcpf(lo * (hi + th)));
  const float yl = y * log1p_c(d * __builtin_amdgcn_rcpf(lo));
  Corr c;
  c.dev = 2.f * ((up ? ya : -ya) - th * ly);
  c.ll = y * (LN2 * (l2mu - l2th) - lm);
  c.pl = y - (up ? yl : -yl);
  return c;
}

// The terms of a count y != 0 that depend on y and theta only, in fp64:
//   cl = lgamma(y + theta) - lgamma(theta) - lgamma(y + 1)      the NB log density's
//   st = lgamma(y + 1) - (y log y - y)                          the Poisson log density's: pll = -(y log(y / mu) - y + mu) - st,
// Stirling's remainder (log(2 pi y) / 2 + ...), so that the rate part of pll is minus half a unit deviance and nothing of
// the size y log y is rounded to fp32.  The gene's table row and the table of st for an integer below TAB, the fp64
// lgamma and log otherwise.
struct Const { double cl, st; };
__device__ __forceinline__ Const const_terms(float y1, const double* row, const double* lf) {
  const int yi = (int)y1;
  if (y1 == (float)yi && yi > 0 && yi < TAB) return Const{row[yi], lf[yi]};
  const double yd = (double)y1, lg = lgamma(yd + 1.0);
  return Const{lgamma(yd + row[TAB + 1]) - row[TAB] - lg, lg - yd * (log(yd) - 1.0)};
}

__global__ __launch_bounds__(256) void nd_vsum_kernel(const float* V, int64_t n, double* out) {
  __shared__ double sh[8];
  double v = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) v += (double)V[i];
  const double t = block_sum(v, sh);
  if (threadIdx.x == 0) out[0] = t;
}

// T [D][TROW]: const_terms' cl for y < TAB, lgamma(theta), theta; lf [TAB]: const_terms' st for y < TAB
__global__ __launch_bounds__(256) void nd_table_kernel(const float* theta, int64_t D, double* T, double* lf) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < TAB) lf[i] = i > 0 ? lgamma((double)i + 1.0) - (double)i * (log((double)i) - 1.0) : 0.0;
  if (i >= D * TROW) return;
  const int64_t d = i / TROW;
  const int j = (int)(i - d * TROW);
  const double th = (double)theta[d];
  double v;
  if (j == TAB + 1) v = th;
  else if (j == TAB) v = lgamma(th);
  else if (th > 1e-20 && th < 1e8) {
    double p = 1.0;
    for (int k = 0; k < j; ++k) p *= th + k;      // <= 1e8^15
    v = log(p) - lgamma((double)j + 1.0);
  } else v = lgamma(th + j) - lgamma(th) - lgamma((double)j + 1.0);
  T[i] = v;
}

// ---------------------------------------------------------------------------------------------------------------------
// dense: the pass over y that forms sum y and the lgamma sums
// ---------------------------------------------------------------------------------------------------------------------

struct ConstArgs {
  const float* y; const double *T, *lf;
  double* gcs;                    // [SN][CQ][D]
  float* cslab;                   // [GB][N]: per spot, sum over the block's genes of const_terms' cl
  int64_t N, D;
  int SN;
};

// grid (ceil(D / 64), SN), 4 waves; wave w owns 16 genes and sweeps its spot slice in tiles of 64, lane = spot: a gene's 64
// counts are one 256-byte read, its sums stay in the lane's registers for the whole sweep.
__global__ __launch_bounds__(256) void nd_const_kernel(ConstArgs a) {
  __shared__ double sT[4][TG][TROW];
  __shared__ double slf[TAB];
  __shared__ double sp[2][4][TS];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t d0 = ((int64_t)blockIdx.x * 4 + wave) * TG;
  for (int i = lane; i < TG * TROW; i += 64) {
    const int g = i / TROW, j = i - g * TROW;
    sT[wave][g][j] = d0 + g < a.D ? a.T[(d0 + g) * TROW + j] : 1.0;
  }
  if (threadIdx.x < TAB) slf[threadIdx.x] = a.lf[threadIdx.x];
  __syncthreads();
  const int64_t ntiles = (a.N + TS - 1) / TS, tper = (ntiles + a.SN - 1) / a.SN;
  const int64_t t_lo = blockIdx.y * tper, t_hi = (t_lo + tper < ntiles) ? t_lo + tper : ntiles;
  double acc[TG][CQ];
#pragma unroll
  for (int g = 0; g < TG; ++g)
#pragma unroll
    for (int k = 0; k < CQ; ++k) acc[g][k] = 0.0;
  int par = 0;
  for (int64_t tt = t_lo; tt < t_hi; ++tt, par ^= 1) {
    const int64_t n0 = tt * TS, n = n0 + lane;
    float yy[TG];
#pragma unroll
    for (int g = 0; g < TG; ++g) yy[g] = (n < a.N && d0 + g < a.D) ? a.y[(d0 + g) * a.N + n] : 0.f;
    double sc = 0.0;
#pragma unroll
    for (int g = 0; g < TG; ++g)
      if (yy[g] != 0.f) {
        const Const c = const_terms(yy[g], sT[wave][g], slf);
        acc[g][0] += (double)yy[g]; acc[g][1] += c.cl; acc[g][2] += c.st;
        sc += c.cl;
      }
    sp[par][wave][lane] = sc;
    // One barrier per tile: the buffer written two tiles ago was read before its readers reached this one.
    __syncthreads();
    if (threadIdx.x < TS && n0 + threadIdx.x < a.N)
      a.cslab[(int64_t)blockIdx.x * a.N + n0 + threadIdx.x] =
          (float)((sp[par][0][threadIdx.x] + sp[par][1][threadIdx.x]) + (sp[par][2][threadIdx.x] + sp[par][3][threadIdx.x]));
  }
#pragma unroll
  for (int g = 0; g < TG; ++g)
#pragma unroll
    for (int k = 0; k < CQ; ++k) {
      const double t = wave_sum(acc[g][k]);
      if (lane == 0 && d0 + g < a.D) a.gcs[((int64_t)blockIdx.y * CQ + k) * a.D + d0 + g] = t;
    }
}

// gc [CQ][D] from the slices (dense) and the null model's rate r_d = sum y / sum V
__global__ __launch_bounds__(256) void nd_rate_kernel(const double* gcs, int SN, int64_t D, const double* vsum, double* gc,
                                                      float* rD) {
  const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (d >= D) return;
  double v[CQ] = {0.0, 0.0, 0.0};
  for (int s = 0; s < SN; ++s)
#pragma unroll
    for (int k = 0; k < CQ; ++k) v[k] += gcs[((int64_t)s * CQ + k) * D + d];
#pragma unroll
  for (int k = 0; k < CQ; ++k) gc[(int64_t)k * D + d] = v[k];
  rD[d] = (float)(v[0] / vsum[0]);
}

// ---------------------------------------------------------------------------------------------------------------------
// the tile pass (dense) and the zero pass (sparse): one kernel, with and without counts
// ---------------------------------------------------------------------------------------------------------------------

struct TileArgs {
  const float *W, *theta, *y;     // y: null in the zero pass
  const float *mF, *Vw, *rD;      // (Lt, N); [Np], V = 1 beyond N; (D,)
  double* gslab;                  // [SN][GQ or ZQ][D]
  float *s0, *s1;                 // [GB][N]: per spot the deviance and the log density's rate part (unused in the zero pass)
  double* zs;                     // [GB][N], the zero pass: per spot z(mu).  fp64, and summed in fp64 over the genes: a stored
                                  // count's correction takes 2 z(mu) back, so at large rates the output is what is left of
                                  // sums a million times its size
  int64_t N, D;
  int Lt, SN;
};

// The sums over the wave's 16 genes of 16 per-lane values: a halving exchange across the gene lanes r (see dv_tile_kernel)
// leaves lane r with the sum over all 16 genes of value r, i.e. of spot 16q + r = the lane's own number in the wave.
template <typename T>
__device__ __forceinline__ T gene_lanes_sum(T (&v)[16], int r) {
  const bool b8 = (r & 8) != 0, b4 = (r & 4) != 0, b2 = (r & 2) != 0, b1 = (r & 1) != 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) { const T keep = b8 ? v[i + 8] : v[i], send = b8 ? v[i] : v[i + 8]; v[i] = keep + __shfl_xor(send, 8); }
#pragma unroll
  for (int i = 0; i < 4; ++i) { const T keep = b4 ? v[i + 4] : v[i], send = b4 ? v[i] : v[i + 4]; v[i] = keep + __shfl_xor(send, 4); }
#pragma unroll
  for (int i = 0; i < 2; ++i) { const T keep = b2 ? v[i + 2] : v[i], send = b2 ? v[i] : v[i + 2]; v[i] = keep + __shfl_xor(send, 2); }
  const T keep = b1 ? v[1] : v[0], send = b1 ? v[0] : v[1];
  return keep + __shfl_xor(send, 1);
}

template <bool ZERO> struct SpotSum { typedef float type; };
template <> struct SpotSum<true> { typedef double type; };

template <int KS, bool ZERO>
__global__ __launch_bounds__(256) void nd_tile_kernel(TileArgs a) {
  constexpr bool PFA = KS <= 8;                 // the A operand of the next tile fits in registers beside the current one
  constexpr int NQ = ZERO ? ZQ : GQ, NS = ZERO ? 1 : 2;
  typedef typename SpotSum<ZERO>::type spt;     // the per-spot sums: fp64 in the zero pass (see TileArgs::zs)
  __shared__ spt sp[2][NS][4][TS];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int64_t d0 = ((int64_t)blockIdx.x * 4 + wave) * TG;
  const int64_t dcol = d0 + r;                  // this lane's gene (a column of the tile)
  const bool dok = dcol < a.D;
  const int64_t ntiles = (a.N + TS - 1) / TS, tper = (ntiles + a.SN - 1) / a.SN;
  const int64_t t_lo = blockIdx.y * tper, t_hi = (t_lo + tper < ntiles) ? t_lo + tper : ntiles;
  const bool vec = !ZERO && (a.N & 3) == 0 && (reinterpret_cast<uintptr_t>(a.y) & 15) == 0;   // rows of y start 16-byte aligned
  // the gene's theta, 1 / theta, log2 theta and null rate (1 for a gene that does not exist: its elements are masked, but
  // the arithmetic must stay finite)
  const float th = dok ? a.theta[dcol] : 1.f, ith = 1.f / th, l2th = __builtin_amdgcn_logf(th);
  const float rd = dok ? a.rD[dcol] : 0.f;
  const bool rpos = rd > 0.f;
  float wb[KS];                                 // B[k = factor 4 ks + q][column = gene r]
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int l = 4 * ks + q;
    wb[ks] = (dok && l < a.Lt) ? a.W[dcol * a.Lt + l] : 0.f;
  }
  const int arow = 16 * (r >> 2) + (r & 3);     // A row r of sub-tile c is spot 16 (r >> 2) + 4c + (r & 3) of the tile
  double gsum[NQ];
#pragma unroll
  for (int k = 0; k < NQ; ++k) gsum[k] = 0.0;
  struct Tile { f4 yv[4], vv[4]; float av[4][KS]; };
  auto load_tile = [&](int64_t tt, Tile& T) __attribute__((always_inline)) {
    const int64_t n0 = tt * TS;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int64_t n = n0 + 16 * q + 4 * c;    // < Np: the padded array covers the tile
      T.vv[c] = *reinterpret_cast<const f4*>(a.Vw + n);
      T.yv[c] = f4{0, 0, 0, 0};
      if (!ZERO && dok) {
        const float* yp = a.y + dcol * a.N + n;
        if (vec && n + 3 < a.N) T.yv[c] = *reinterpret_cast<const f4*>(yp);
        else {
#pragma unroll
          for (int g = 0; g < 4; ++g) if (n + g < a.N) T.yv[c][g] = yp[g];
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
        T.av[c][ks] = (l < a.Lt && na < a.N) ? a.mF[(int64_t)l * a.N + na] : 0.f;
      }
    }
  };
  Tile cur, nxt;
  if (t_lo < t_hi) { load_tile(t_lo, cur); if (PFA) load_a(t_lo, cur); }
  nxt = cur;
  int par = 0;
  for (int64_t tt = t_lo; tt < t_hi; ++tt, par ^= 1) {
    const int64_t n0 = tt * TS;
    if (!PFA) load_a(tt, cur);
    if (tt + 1 < t_hi) { load_tile(tt + 1, nxt); if (PFA) load_a(tt + 1, nxt); }
    // rate tile: row 4q + g of sub-tile c is spot 16q + 4c + g, column r is gene d0 + r
    f4 z[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      z[c] = f4{0, 0, 0, 0};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) z[c] = mfma4(cur.av[c][ks], wb[ks], z[c]);
    }
    float f[NQ];
#pragma unroll
    for (int k = 0; k < NQ; ++k) f[k] = 0.f;
    spt v[16];                                  // [4c + g]: the element at spot 16q + 4c + g of gene d0 + r
    float w[16];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const bool ok = dok && n0 + 16 * q + 4 * c + g < a.N;
        const float vn = cur.vv[c][g];
        const float mu = ok ? vn * z[c][g] : 1.f;
        const float lm = log1p_c(mu * ith);     // log1p(mu / theta)
        if constexpr (ZERO) {
          const float zz = ok ? th * lm : 0.f;
          f[0] += zz; f[1] += ok ? mu : 0.f; f[2] += (ok && rpos) ? th * log1p_c(vn * rd * ith) : 0.f;
          v[4 * c + g] = zz;
        } else {
          const float y1 = cur.yv[c][g];        // 0 where the element does not exist
          const float l2mu = __builtin_amdgcn_logf(mu);
          const Unit un = unit_dev(y1, mu, th);
          const float dev = ok ? un.dev : 0.f;
          const float ylm = y1 * LN2 * l2mu;    // y log mu
          const float ll = ok ? __builtin_fmaf(-(y1 + th), lm, __builtin_fmaf(-y1 * LN2, l2th, ylm)) : 0.f;
          const float mu0 = (ok && rpos) ? vn * rd : 1.f;
          const float dev0 = (ok && rpos) ? unit_dev(y1, mu0, th).dev : 0.f;
          // the Poisson log density's rate part: -(y log(y / mu) - (y - mu)), the rest is const_terms' st
          f[0] += dev; f[1] += ok ? mu : 0.f; f[2] += dev0; f[3] += ll; f[4] += ok ? (y1 - mu) - un.yl : 0.f;
          v[4 * c + g] = dev;
          w[4 * c + g] = ll;
        }
      }
#pragma unroll
    for (int k = 0; k < NQ; ++k) gsum[k] += (double)f[k];
    sp[par][0][wave][lane] = gene_lanes_sum(v, r);
    if constexpr (!ZERO) sp[par][1][wave][lane] = gene_lanes_sum(w, r);
    // One barrier per tile: the buffer written two tiles ago was read before its readers reached this one.
    __syncthreads();
    if (threadIdx.x < NS * TS) {
      const int k = threadIdx.x >> 6, t = threadIdx.x & 63;      // k is uniform over the wave
      if (n0 + t < a.N) {
        const spt sum = (sp[par][k][0][t] + sp[par][k][1][t]) + (sp[par][k][2][t] + sp[par][k][3][t]);
        if constexpr (ZERO) a.zs[(int64_t)blockIdx.x * a.N + n0 + t] = sum;
        else (k == 0 ? a.s0 : a.s1)[(int64_t)blockIdx.x * a.N + n0 + t] = sum;
      }
    }
    cur = nxt;
  }
  // the gene's sums over this slice: the four spot groups q in a fixed order, lanes q == 0 write
#pragma unroll
  for (int k = 0; k < NQ; ++k) {
    double t = gsum[k];
    t += __shfl_xor(t, 16); t += __shfl_xor(t, 32);
    if (q == 0 && dok) a.gslab[((int64_t)blockIdx.y * NQ + k) * a.D + dcol] = t;
  }
}

// Every per-gene output and the workgroup's partials of the scalars.  gslab [SN][GQ][D], gc [CQ][D].
__global__ __launch_bounds__(256) void nd_finish_kernel(const double* gslab, int SN, const double* gc, int64_t D,
                                                        double* per_gene, double* null_per_gene, double* ll_per_gene,
                                                        double* pll_per_gene, double* partial) {
  __shared__ double sh[8];
  const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double g[GQ] = {0.0, 0.0, 0.0, 0.0, 0.0}, sy = 0.0, nul = 0.0, ll = 0.0, pl = 0.0;
  if (d < D) {
    for (int s = 0; s < SN; ++s)
#pragma unroll
      for (int k = 0; k < GQ; ++k) g[k] += gslab[((int64_t)s * GQ + k) * D + d];
    sy = gc[d];
    nul = sy > 0.0 ? g[2] : 0.0;
    ll = g[3] + gc[D + d];                      // const_terms' cl and st
    pl = g[4] - gc[2 * D + d];
    per_gene[d] = g[0];
    null_per_gene[d] = nul;
    ll_per_gene[d] = ll;
    pll_per_gene[d] = pl;
  }
  const double t[NSCAL] = {block_sum(g[0], sh), block_sum(sy, sh), block_sum(g[1], sh), block_sum(nul, sh), block_sum(ll, sh),
                           block_sum(pl, sh)};
  if (threadIdx.x == 0) {
    double* p = partial + (int64_t)blockIdx.x * NSCAL;
#pragma unroll
    for (int k = 0; k < NSCAL; ++k) p[k] = t[k];
  }
}

__global__ __launch_bounds__(256) void nd_total_kernel(const double* partial, int64_t nb, double* scalars) {
  __shared__ double sh[8];
  double v[NSCAL] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t b = threadIdx.x; b < nb; b += 256)
#pragma unroll
    for (int k = 0; k < NSCAL; ++k) v[k] += partial[b * NSCAL + k];
#pragma unroll
  for (int k = 0; k < NSCAL; ++k) {
    const double t = block_sum(v[k], sh);
    if (threadIdx.x == 0) scalars[k] = t;
  }
}

// per spot: the gene blocks' slabs in order.  per_spot = fa sum s0 + (ca ? ca[n] : 0);
// ll_per_spot = fb sum sb + sum sc + (cb ? cb[n] : 0)   (sc nullable)
template <typename T>
__global__ __launch_bounds__(256) void nd_spot_sum_kernel(const T* s0, const T* sb, const float* sc, int GB, int64_t N,
                                                          double fa, double fb, const double* ca, const double* cb,
                                                          double* per_spot, double* ll_per_spot) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  double v = 0.0, u = 0.0, c = 0.0;
#pragma unroll 4
  for (int b = 0; b < GB; ++b) {
    v += (double)s0[(int64_t)b * N + n];
    u += (double)sb[(int64_t)b * N + n];
    if (sc) c += (double)sc[(int64_t)b * N + n];
  }
  per_spot[n] = fa * v + (ca ? ca[n] : 0.0);
  ll_per_spot[n] = (fb * u + c) + (cb ? cb[n] : 0.0);
}

static int ksteps(int Lt) {                     // the instances of deviance.hip: k-steps of 4 factors
  const int k = (Lt + 3) / 4;
  return k <= 10 ? k : k <= 12 ? 12 : k <= 14 ? 14 : 16;
}

struct Slices { int SN, GB, KS; int64_t tper, Np, nbD; };

static Slices slices(int64_t N, int64_t D, int Lt) {
  Slices p;
  const int64_t ntiles = (N + TS - 1) / TS;
  p.GB = (int)((D + BG - 1) / BG);
  // enough (gene block, spot slice) workgroups to fill the device a few times over, slices of at least 8 tiles
  int64_t SN = (1024 + p.GB - 1) / p.GB;
  if (SN > (N + 511) / 512) SN = (N + 511) / 512;
  if (SN > 16) SN = 16;
  if (SN < 1) SN = 1;
  p.SN = (int)SN;
  p.tper = (ntiles + SN - 1) / SN;
  p.Np = ntiles * TS;
  p.KS = ksteps(Lt);
  p.nbD = (D + 255) / 256;
  return p;
}

template <bool ZERO>
static void launch_tiles(int KS, const TileArgs& a, int GB, hipStream_t s) {
  const dim3 grid((unsigned)GB, (unsigned)a.SN), block(256);
  switch (KS) {
    case 1: hipLaunchKernelGGL((nd_tile_kernel<1, ZERO>), grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL((nd_tile_kernel<2, ZERO>), grid, block, 0, s, a); break;
    case 3: hipLaunchKernelGGL((nd_tile_kernel<3, ZERO>), grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL((nd_tile_kernel<4, ZERO>), grid, block, 0, s, a); break;
    case 5: hipLaunchKernelGGL((nd_tile_kernel<5, ZERO>), grid, block, 0, s, a); break;
    case 6: hipLaunchKernelGGL((nd_tile_kernel<6, ZERO>), grid, block, 0, s, a); break;
    case 7: hipLaunchKernelGGL((nd_tile_kernel<7, ZERO>), grid, block, 0, s, a); break;
    case 8: hipLaunchKernelGGL((nd_tile_kernel<8, ZERO>), grid, block, 0, s, a); break;
    case 9: hipLaunchKernelGGL((nd_tile_kernel<9, ZERO>), grid, block, 0, s, a); break;
    case 10: hipLaunchKernelGGL((nd_tile_kernel<10, ZERO>), grid, block, 0, s, a); break;
    case 12: hipLaunchKernelGGL((nd_tile_kernel<12, ZERO>), grid, block, 0, s, a); break;
    case 14: hipLaunchKernelGGL((nd_tile_kernel<14, ZERO>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL((nd_tile_kernel<16, ZERO>), grid, block, 0, s, a); break;
  }
}

// m (Lt, N) and V padded to whole tiles (1 beyond N); mT [N][LT] (zeros beyond Lt) when asked for
__global__ __launch_bounds__(256) void nd_factors_kernel(const float* mean, const float* scale, const float* V, int64_t N,
                                                         int64_t Np, int Lt, int LT, int lognormal, float* mF, float* Vw,
                                                         float* mT) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (int64_t)Lt * N) {
    const float s = scale[i];
    mF[i] = expf(mean[i] + (lognormal ? 0.5f * s * s : 0.f));
  }
  if (i < Np) Vw[i] = i < N ? V[i] : 1.f;
  if (mT && i < N * LT) {
    const int64_t j = i / LT;
    const int l = (int)(i - j * LT);
    float m = 0.f;
    if (l < Lt) {
      const float s = scale[(int64_t)l * N + j];
      m = expf(mean[(int64_t)l * N + j] + (lognormal ? 0.5f * s * s : 0.f));
    }
    mT[i] = m;
  }
}

struct DensePlan {
  Slices sl; size_t bytes;
  float *mF, *Vw, *cslab, *rD, *s0, *s1;
  double *vsum, *T, *lf, *gcs, *gc, *gslab, *partial;
};

static DensePlan dense_plan(int64_t N, int64_t D, int Lt, void* ws) {
  DensePlan p;
  p.sl = slices(N, D, Lt);
  Carver c(ws);
  p.mF = c.take<float>((size_t)Lt * N);
  p.Vw = c.take<float>((size_t)p.sl.Np);
  p.vsum = c.take<double>(1);
  p.T = c.take<double>((size_t)D * TROW);
  p.lf = c.take<double>(TAB);
  p.gcs = c.take<double>((size_t)p.sl.SN * CQ * D);
  p.gc = c.take<double>((size_t)CQ * D);
  p.rD = c.take<float>((size_t)D);
  p.cslab = c.take<float>((size_t)p.sl.GB * N);
  p.gslab = c.take<double>((size_t)p.sl.SN * GQ * D);
  p.s0 = c.take<float>((size_t)p.sl.GB * N);
  p.s1 = c.take<float>((size_t)p.sl.GB * N);
  p.partial = c.take<double>((size_t)p.sl.nbD * NSCAL);
  p.bytes = c.used();
  return p;
}

static int check_shape(const char* who, int64_t N, int64_t D, int Lt) {
  GPZ_REQUIRE(N >= 1 && D >= 1, "%s: bad extents (N = %lld, D = %lld)", who, (long long)N, (long long)D);
  GPZ_REQUIRE(Lt >= 1 && Lt <= MAXL, "%s: %d factors unsupported (1..%d)", who, Lt, MAXL);
  GPZ_REQUIRE(N < (1ll << 31) && D < (1ll << 31), "%s: spots and genes are indexed with 32 bits", who);
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// sparse
// ---------------------------------------------------------------------------------------------------------------------

struct SpArgs {
  const float *W, *V, *theta;
  const int64_t* col_ptr; const int32_t* col_gene; const float* col_val;
  const int64_t* row_ptr; const int32_t* row_spot; const int32_t* row_perm;
  const int32_t *idx, *pos;
  const float *mT, *rD;           // [B][LT] (zeros beyond Lt), (D,)
  const double *T, *lf, *vsum;
  int32_t *cstart, *chunk_gene;   // [D + 1], [nchunks]
  double* part0;                  // [nchunks][CQ]
  double* part;                   // [nchunks][4]: the corrections of the deviance, ll, pll and the null deviance
  double* spc;                    // [2][B]: a spot's corrections of the deviance and of ll
  double *gc, *zgs, *gslab;       // [CQ][D], [SN][ZQ][D], [GQ][D]
  int64_t N, B, D, nnz, nchunks;
  int Lt, LT, SN;
};

static int instance(int Lt) {
  const int sizes[] = {4, 8, 12, 16, 20, 24, 32, 40, 48, 64};
  for (int s : sizes) if (Lt <= s) return s;
  return 0;
}

// 4 waves per workgroup, wave = chunk w: sum y and the lgamma sums over the chunk's entries that lie in the batch
__global__ __launch_bounds__(256) void nds_const_kernel(SpArgs a) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t wi = (int64_t)blockIdx.x * 4 + wave;
  if (wi >= a.nchunks) return;              // no barrier below
  const int g = a.chunk_gene[wi];
  double s[CQ] = {0.0, 0.0, 0.0};
  if (g >= 0) {
    const int64_t p0 = a.row_ptr[g] + (wi - a.cstart[g]) * CHUNK;
    const int64_t pe = a.row_ptr[g + 1], p1 = p0 + CHUNK < pe ? p0 + CHUNK : pe;
    const double* row = a.T + (int64_t)g * TROW;
    for (int64_t p = p0 + lane; p < p1; p += 64) {
      const int n = a.row_spot[p];
      const int j = a.pos ? a.pos[n] : n;
      if (j < 0) continue;
      const float y = a.col_val[a.row_perm[p]];
      if (y == 0.f) continue;
      const Const c = const_terms(y, row, a.lf);
      s[0] += (double)y; s[1] += c.cl; s[2] += c.st;
    }
  }
#pragma unroll
  for (int k = 0; k < CQ; ++k) {
    const double t = wave_sum(s[k]);
    if (lane == 0) a.part0[wi * CQ + k] = t;
  }
}

// gc [CQ][D] from the row's chunk partials in chunk order, and r_d
__global__ __launch_bounds__(256) void nds_rate_kernel(SpArgs a, float* rD) {
  const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (d >= a.D) return;
  double v[CQ] = {0.0, 0.0, 0.0};
  for (int64_t c = a.cstart[d]; c < a.cstart[d + 1]; ++c)
#pragma unroll
    for (int k = 0; k < CQ; ++k) v[k] += a.part0[c * CQ + k];
#pragma unroll
  for (int k = 0; k < CQ; ++k) a.gc[(int64_t)k * a.D + d] = v[k];
  rD[d] = (float)(v[0] / a.vsum[0]);
}

// Spot pass.  4 waves per workgroup, wave = batch spot j (global spot n = idx[j]); lanes stride over the column's
// non-zeros.  No barrier.
template <int LT>
__global__ __launch_bounds__(256) void nds_spot_kernel(SpArgs a) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t j = (int64_t)blockIdx.x * 4 + wave;
  if (j >= a.B) return;
  const int64_t n = a.idx ? a.idx[j] : j;
  const int64_t k0 = a.col_ptr[n], k1 = a.col_ptr[n + 1];
  const float vn = a.V[j];
  float m[LT];
  const f4* mp = reinterpret_cast<const f4*>(a.mT + j * LT);
#pragma unroll
  for (int l = 0; l < LT; l += 4) {
    const f4 v = mp[l / 4];
    m[l] = v[0]; m[l + 1] = v[1]; m[l + 2] = v[2]; m[l + 3] = v[3];
  }
  double ad = 0.0, al = 0.0;
  for (int64_t k = k0 + lane; k < k1; k += 64) {
    const float y = a.col_val[k];
    if (y == 0.f) continue;                 // an explicit zero: the zero part is all of it
    const int g = a.col_gene[k];
    float w[LT];
    load_w<LT>(a.W, g, a.Lt, w);
    float z = 0.f;
#pragma unroll
    for (int l = 0; l < LT; ++l) z = __builtin_fmaf(w[l], m[l], z);
    const float th = a.theta[g];
    const Corr c = stored_corr(y, vn * z, th, 1.f / th, __builtin_amdgcn_logf(th));
    const Const t = const_terms(y, a.T + (int64_t)g * TROW, a.lf);
    ad += (double)c.dev;
    al += (double)c.ll + t.cl;
  }
  ad = wave_sum(ad);
  al = wave_sum(al);
  if (lane == 0) { a.spc[j] = ad; a.spc[a.B + j] = al; }
}

// Gene pass.  4 waves per workgroup, wave = chunk w of the work list.  The wave packs the chunk's entries that lie in
// the batch (pos[n] >= 0) and are not stored zeros into LDS, in their order, then every lane takes every 64th packed entry.
template <int LT>
__global__ __launch_bounds__(256) void nds_gene_kernel(SpArgs a) {
  __shared__ int32_t lj[4][CHUNK];
  __shared__ float ly[4][CHUNK];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t wi = (int64_t)blockIdx.x * 4 + wave;
  const int g = wi < a.nchunks ? a.chunk_gene[wi] : -1;
  int cnt = 0;
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
      const unsigned long long mk = __ballot(keep);
      if (keep) {
        const int at = cnt + __popcll(mk & ((1ull << lane) - 1ull));
        lj[wave][at] = j;
        ly[wave][at] = y;
      }
      cnt += __popcll(mk);
    }
  }
  __syncthreads();                 // every wave, with or without a chunk, arrives here exactly once
  if (g < 0) return;
  float w[LT];
  load_w<LT>(a.W, g, a.Lt, w);
  const float th = a.theta[g], ith = 1.f / th, l2th = __builtin_amdgcn_logf(th), rd = a.rD[g];
  float acc[4] = {0.f, 0.f, 0.f, 0.f};           // at most 8 entries per lane
  for (int i = lane; i < cnt; i += 64) {
    const int64_t j = lj[wave][i];
    const float y = ly[wave][i];
    const f4* mp = reinterpret_cast<const f4*>(a.mT + j * LT);
    float z = 0.f;
#pragma unroll
    for (int l = 0; l < LT; l += 4) {
      const f4 v = mp[l / 4];
      z = __builtin_fmaf(w[l], v[0], z); z = __builtin_fmaf(w[l + 1], v[1], z);
      z = __builtin_fmaf(w[l + 2], v[2], z); z = __builtin_fmaf(w[l + 3], v[3], z);
    }
    const float vj = a.V[j];
    const Corr c = stored_corr(y, vj * z, th, ith, l2th);
    const Corr c0 = stored_corr(y, vj * rd, th, ith, l2th);    // rd > 0: the row has a count in the batch
    acc[0] += c.dev; acc[1] += c.ll; acc[2] += c.pl; acc[3] += c0.dev;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double t = wave_sum((double)acc[k]);
    if (lane == 0) a.part[wi * 4 + k] = t;
  }
}

// gslab [GQ][D]: the zero pass's slices in order plus the row's chunk partials in chunk order
__global__ __launch_bounds__(256) void nds_gene_finish_kernel(SpArgs a) {
  const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (d >= a.D) return;
  double z[ZQ] = {0.0, 0.0, 0.0}, v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int s = 0; s < a.SN; ++s)
#pragma unroll
    for (int k = 0; k < ZQ; ++k) z[k] += a.zgs[((int64_t)s * ZQ + k) * a.D + d];
  for (int64_t c = a.cstart[d]; c < a.cstart[d + 1]; ++c)
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] += a.part[c * 4 + k];
  a.gslab[d] = 2.0 * z[0] + v[0];
  a.gslab[a.D + d] = z[1];
  a.gslab[2 * a.D + d] = 2.0 * z[2] + v[3];
  a.gslab[3 * a.D + d] = v[1] - z[0];
  a.gslab[4 * a.D + d] = v[2] - z[1];
}

struct SpPlan {
  Slices sl; int LT; int64_t nchunks; size_t bytes;
  float *mF, *Vw, *mT, *rD;
  double *zslab, *vsum, *T, *lf, *part0, *part, *spc, *gc, *zgs, *gslab, *partial;
  int32_t *cstart, *chunk_gene;
};

static SpPlan sp_plan(int64_t B, int64_t D, int Lt, int64_t nnz, void* ws) {
  SpPlan p;
  p.sl = slices(B, D, Lt);
  p.LT = instance(Lt);
  p.nchunks = D + nnz / CHUNK;               // sum_d ceil(len_d / C) <= D + floor(nnz / C)
  Carver c(ws);
  p.mF = c.take<float>((size_t)Lt * B);
  p.Vw = c.take<float>((size_t)p.sl.Np);
  p.mT = c.take<float>((size_t)B * p.LT);
  p.vsum = c.take<double>(1);
  p.T = c.take<double>((size_t)D * TROW);
  p.lf = c.take<double>(TAB);
  p.cstart = c.take<int32_t>((size_t)D + 1);
  p.chunk_gene = c.take<int32_t>((size_t)p.nchunks);
  p.part0 = c.take<double>((size_t)p.nchunks * CQ);
  p.part = c.take<double>((size_t)p.nchunks * 4);
  p.spc = c.take<double>((size_t)2 * B);
  p.gc = c.take<double>((size_t)CQ * D);
  p.rD = c.take<float>((size_t)D);
  p.zgs = c.take<double>((size_t)p.sl.SN * ZQ * D);
  p.zslab = c.take<double>((size_t)p.sl.GB * B);
  p.gslab = c.take<double>((size_t)GQ * D);
  p.partial = c.take<double>((size_t)p.sl.nbD * NSCAL);
  p.bytes = c.used();
  return p;
}

static int sp_check_shape(const char* who, int64_t N, int64_t B, int64_t D, int Lt, int64_t nnz) {
  GPZ_REQUIRE(N >= 1 && B >= 1 && D >= 1 && nnz >= 0, "%s: bad extents (N = %lld, B = %lld, D = %lld, nnz = %lld)", who,
              (long long)N, (long long)B, (long long)D, (long long)nnz);
  GPZ_REQUIRE(B <= N, "%s: a batch of %lld distinct spots out of %lld", who, (long long)B, (long long)N);
  GPZ_REQUIRE(Lt >= 1 && Lt <= MAXL, "%s: %d factors unsupported (1..%d)", who, Lt, MAXL);
  GPZ_REQUIRE(N < (1ll << 31) && D < (1ll << 31) && nnz < (1ll << 31) && D + nnz / CHUNK < (1ll << 31),
              "%s: spots, genes and non-zeros are indexed with 32 bits", who);
  return 0;
}

template <int LT>
static int sp_passes(const SpArgs& a, hipStream_t s) {
  hipLaunchKernelGGL((nds_spot_kernel<LT>), dim3((unsigned)((a.B + 3) / 4)), dim3(256), 0, s, a);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL((nds_gene_kernel<LT>), dim3((unsigned)((a.nchunks + 3) / 4)), dim3(256), 0, s, a);
  GPZ_LAUNCH_OK();
  return 0;
}

}  // namespace nbd
}  // namespace gpz

using namespace gpz;
using namespace gpz::nbd;

extern "C" int gpz_nb_deviance_plan(int64_t N, int64_t D, int32_t Lt, int32_t* spots_per_tile, int32_t* genes_per_tile,
                                    int32_t* genes_per_block, int32_t* gene_slices, int32_t* spot_slices,
                                    int64_t* tiles_per_spot_slice, int32_t* factors_padded) {
  if (int rc = check_shape("gpz_nb_deviance_plan", N, D, Lt)) return rc;
  const Slices p = slices(N, D, Lt);
  if (spots_per_tile) *spots_per_tile = TS;
  if (genes_per_tile) *genes_per_tile = TG;
  if (genes_per_block) *genes_per_block = BG;
  if (gene_slices) *gene_slices = p.GB;
  if (spot_slices) *spot_slices = p.SN;
  if (tiles_per_spot_slice) *tiles_per_spot_slice = p.tper;
  if (factors_padded) *factors_padded = 4 * p.KS;
  return 0;
}

extern "C" size_t gpz_nb_deviance_workspace_bytes(int64_t N, int64_t D, int32_t Lt) {
  if (check_shape("gpz_nb_deviance_workspace_bytes", N, D, Lt)) return 0;
  return dense_plan(N, D, Lt, nullptr).bytes;
}

extern "C" int gpz_nb_deviance(const float* mean, const float* scale, const float* W, const float* V, const float* theta,
                               const float* y, int64_t N, int64_t D, int32_t Lt, int32_t lognormal_mean, double* per_gene,
                               double* per_spot, double* null_per_gene, double* loglik_per_gene, double* loglik_per_spot,
                               double* poisson_loglik_per_gene, double* scalars, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_shape("gpz_nb_deviance", N, D, Lt)) return rc;
  GPZ_REQUIRE(theta, "gpz_nb_deviance: theta is missing (null pointer)");
  GPZ_REQUIRE(mean && scale && W && V && y && per_gene && per_spot && null_per_gene && loglik_per_gene && loglik_per_spot &&
                  poisson_loglik_per_gene && scalars && ws,
              "gpz_nb_deviance: null pointer");
  GPZ_REQUIRE(((reinterpret_cast<uintptr_t>(W) | reinterpret_cast<uintptr_t>(ws)) & 15) == 0,
              "gpz_nb_deviance: W and the workspace must be 16-byte aligned");
  const DensePlan p = dense_plan(N, D, Lt, ws);
  GPZ_REQUIRE(ws_bytes >= p.bytes, "gpz_nb_deviance: workspace of %zu bytes, %zu needed", ws_bytes, p.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const Slices& sl = p.sl;
  const int64_t tot = (int64_t)Lt * N > sl.Np ? (int64_t)Lt * N : sl.Np;
  hipLaunchKernelGGL(nd_factors_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, mean, scale, V, N, sl.Np, (int)Lt,
                     0, (int)(lognormal_mean != 0), p.mF, p.Vw, (float*)nullptr);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(nd_vsum_kernel, dim3(1), dim3(256), 0, s, V, N, p.vsum);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(nd_table_kernel, dim3((unsigned)((D * TROW + 255) / 256)), dim3(256), 0, s, theta, D, p.T, p.lf);
  GPZ_LAUNCH_OK();
  ConstArgs ca;
  ca.y = y; ca.T = p.T; ca.lf = p.lf; ca.gcs = p.gcs; ca.cslab = p.cslab; ca.N = N; ca.D = D; ca.SN = sl.SN;
  hipLaunchKernelGGL(nd_const_kernel, dim3((unsigned)sl.GB, (unsigned)sl.SN), dim3(256), 0, s, ca);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(nd_rate_kernel, dim3((unsigned)sl.nbD), dim3(256), 0, s, p.gcs, sl.SN, D, p.vsum, p.gc, p.rD);
  GPZ_LAUNCH_OK();
  TileArgs ta;
  ta.W = W; ta.theta = theta; ta.y = y; ta.mF = p.mF; ta.Vw = p.Vw; ta.rD = p.rD; ta.gslab = p.gslab; ta.s0 = p.s0; ta.s1 = p.s1;
  ta.zs = nullptr; ta.N = N; ta.D = D; ta.Lt = Lt; ta.SN = sl.SN;
  launch_tiles<false>(sl.KS, ta, sl.GB, s);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(nd_finish_kernel, dim3((unsigned)sl.nbD), dim3(256), 0, s, p.gslab, sl.SN, p.gc, D, per_gene, null_per_gene,
                     loglik_per_gene, poisson_loglik_per_gene, p.partial);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(nd_spot_sum_kernel<float>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, (const float*)p.s0,
                     (const float*)p.s1, (const float*)p.cslab, sl.GB, N, 1.0,
                     1.0, (const double*)nullptr, (const double*)nullptr, per_spot, loglik_per_spot);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(nd_total_kernel, dim3(1), dim3(256), 0, s, p.partial, sl.nbD, scalars);
  GPZ_LAUNCH_OK();
  return 0;
}

extern "C" int gpz_nb_deviance_sparse_plan(int64_t N, int64_t B, int64_t D, int32_t Lt, int64_t nnz, int32_t* gene_chunk,
                                           int32_t* spot_chunk, int64_t* n_gene_chunks, int32_t* factors_padded) {
  if (int rc = sp_check_shape("gpz_nb_deviance_sparse_plan", N, B, D, Lt, nnz)) return rc;
  if (gene_chunk) *gene_chunk = CHUNK;
  if (spot_chunk) *spot_chunk = 0;
  if (n_gene_chunks) *n_gene_chunks = D + nnz / CHUNK;
  if (factors_padded) *factors_padded = instance(Lt);
  return 0;
}

extern "C" size_t gpz_nb_deviance_sparse_workspace_bytes(int64_t N, int64_t B, int64_t D, int64_t nnz, int32_t Lt) {
  if (sp_check_shape("gpz_nb_deviance_sparse_workspace_bytes", N, B, D, Lt, nnz)) return 0;
  return sp_plan(B, D, Lt, nnz, nullptr).bytes;
}

extern "C" int gpz_nb_deviance_sparse(const float* mean, const float* scale, const float* W, const float* V, const float* theta,
                                      const int64_t* col_ptr, const int32_t* col_gene, const float* col_val,
                                      const int64_t* row_ptr, const int32_t* row_spot, const int32_t* row_perm,
                                      const int32_t* idx, const int32_t* pos, int64_t N, int64_t B, int64_t D, int64_t nnz,
                                      int32_t Lt, int32_t lognormal_mean, double* per_gene, double* per_spot,
                                      double* null_per_gene, double* loglik_per_gene, double* loglik_per_spot,
                                      double* poisson_loglik_per_gene, double* scalars, void* ws, size_t ws_bytes,
                                      void* stream) {
  if (int rc = sp_check_shape("gpz_nb_deviance_sparse", N, B, D, Lt, nnz)) return rc;
  GPZ_REQUIRE(theta, "gpz_nb_deviance_sparse: theta is missing (null pointer)");
  GPZ_REQUIRE(mean && scale && W && V && col_ptr && row_ptr && per_gene && per_spot && null_per_gene && loglik_per_gene &&
                  loglik_per_spot && poisson_loglik_per_gene && scalars && ws,
              "gpz_nb_deviance_sparse: null pointer");
  GPZ_REQUIRE(nnz == 0 || (col_gene && col_val && row_spot && row_perm), "gpz_nb_deviance_sparse: null pointer (non-zeros)");
  GPZ_REQUIRE((idx == nullptr) == (pos == nullptr), "gpz_nb_deviance_sparse: idx and pos come together (both null: all spots)");
  GPZ_REQUIRE(idx || B == N, "gpz_nb_deviance_sparse: B = %lld of N = %lld spots needs idx and pos", (long long)B, (long long)N);
  GPZ_REQUIRE(((reinterpret_cast<uintptr_t>(W) | reinterpret_cast<uintptr_t>(ws)) & 15) == 0,
              "gpz_nb_deviance_sparse: W and the workspace must be 16-byte aligned");
  const SpPlan p = sp_plan(B, D, Lt, nnz, ws);
  GPZ_REQUIRE(ws_bytes >= p.bytes, "gpz_nb_deviance_sparse: workspace of %zu bytes, %zu needed", ws_bytes, p.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const Slices& sl = p.sl;
  SpArgs a;
  a.W = W; a.V = V; a.theta = theta;
  a.col_ptr = col_ptr; a.col_gene = col_gene; a.col_val = col_val;
  a.row_ptr = row_ptr; a.row_spot = row_spot; a.row_perm = row_perm; a.idx = idx; a.pos = pos;
  a.mT = p.mT; a.rD = p.rD; a.T = p.T; a.lf = p.lf; a.vsum = p.vsum; a.cstart = p.cstart; a.chunk_gene = p.chunk_gene;
  a.part0 = p.part0; a.part = p.part; a.spc = p.spc; a.gc = p.gc; a.zgs = p.zgs; a.gslab = p.gslab;
  a.N = N; a.B = B; a.D = D; a.nnz = nnz; a.nchunks = p.nchunks; a.Lt = Lt; a.LT = p.LT; a.SN = sl.SN;
  int64_t tot = (int64_t)Lt * B > sl.Np ? (int64_t)Lt * B : sl.Np;
  if (tot < B * p.LT) tot = B * p.LT;
  hipLaunchKernelGGL(nd_factors_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, mean, scale, V, B, sl.Np, (int)Lt,
                     p.LT, (int)(lognormal_mean != 0), p.mF, p.Vw, p.mT);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(nd_vsum_kernel, dim3(1), dim3(256), 0, s, V, B, p.vsum);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(nd_table_kernel, dim3((unsigned)((D * TROW + 255) / 256)), dim3(256), 0, s, theta, D, p.T, p.lf);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(chunks_kernel, dim3(1), dim3(1024), 0, s, a.row_ptr, a.D, a.nchunks, CHUNK, false, a.cstart, a.chunk_gene);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(nds_const_kernel, dim3((unsigned)((a.nchunks + 3) / 4)), dim3(256), 0, s, a);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(nds_rate_kernel, dim3((unsigned)sl.nbD), dim3(256), 0, s, a, p.rD);
  GPZ_LAUNCH_OK();
  TileArgs ta;
  ta.W = W; ta.theta = theta; ta.y = nullptr; ta.mF = p.mF; ta.Vw = p.Vw; ta.rD = p.rD; ta.gslab = p.zgs; ta.s0 = nullptr;
  ta.s1 = nullptr; ta.zs = p.zslab; ta.N = B; ta.D = D; ta.Lt = Lt; ta.SN = sl.SN;
  launch_tiles<true>(sl.KS, ta, sl.GB, s);
  GPZ_LAUNCH_OK();
  int rc;
  switch (a.LT) {
    case 4: rc = sp_passes<4>(a, s); break;
    case 8: rc = sp_passes<8>(a, s); break;
    case 12: rc = sp_passes<12>(a, s); break;
    case 16: rc = sp_passes<16>(a, s); break;
    case 20: rc = sp_passes<20>(a, s); break;
    case 24: rc = sp_passes<24>(a, s); break;
    case 32: rc = sp_passes<32>(a, s); break;
    case 40: rc = sp_passes<40>(a, s); break;
    case 48: rc = sp_passes<48>(a, s); break;
    default: rc = sp_passes<64>(a, s); break;
  }
  if (rc) return rc;
  hipLaunchKernelGGL(nds_gene_finish_kernel, dim3((unsigned)sl.nbD), dim3(256), 0, s, a);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(nd_finish_kernel, dim3((unsigned)sl.nbD), dim3(256), 0, s, p.gslab, 1, p.gc, D, per_gene, null_per_gene,
                     loglik_per_gene, poisson_loglik_per_gene, p.partial);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(nd_spot_sum_kernel<double>, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, (const double*)p.zslab,
                     (const double*)p.zslab, (const float*)nullptr,
                     sl.GB, B, 2.0, -1.0, (const double*)p.spc, (const double*)(p.spc + B), per_spot, loglik_per_spot);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(nd_total_kernel, dim3(1), dim3(256), 0, s, p.partial, sl.nbD, scalars);
  GPZ_LAUNCH_OK();
  return 0;
}
