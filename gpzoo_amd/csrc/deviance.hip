// deviance.hip -- Poisson deviance of counts under the predictive mean rate of a fitted NSF factor model, per gene, per
// spot and in total, with the null model's deviance beside it; dense counts and counts stored as their non-zeros.  The
// (D, N) rate never exists in HBM.  The reference has no such function (its Dval of anndata_to_train_val is never scored).
//
//   m[l,n]    = exp(mean[l,n] + scale[l,n]^2 / 2)       (E_q[exp F], the lognormal mean; exp(mean) without the flag)
//   mu[d,n]   = V[n] sum_l W[d,l] m[l,n]
//   dev[d,n]  = 2 (y log(y / mu) - y + mu),  the log term exactly 0 at y = 0 (0 log 0 is never formed)
//   per_gene[d] = sum_n dev,  per_spot[n] = sum_d dev,  scalars = {total, sum y, sum mu, null total}
//   null model mu0[d,n] = V[n] r_d, r_d = sum_n y[d,n] / sum_n V[n]:
//   null_per_gene[d] = 2 (sum_n y log y - sum_n y log V[n] - Sy log r_d), Sy = sum_n y[d,n]  (-y + mu0 sums to zero);
//                      exactly 0 where Sy = 0
//
// Dense (gpz_poisson_deviance), fp32 element-wise work, fp64 sums, no atomics, no workgroup waits on another, every sum in
// a fixed order -> two calls agree bit for bit:
//   dv_factors_kernel  m (Lt, N); V and log V padded to whole tiles
//   dv_vsum_kernel     sum_n V[n] (one workgroup)
//   dv_tile_kernel     grid (ceil(D / 64), spot slices), 4 waves; wave w owns 16 genes and sweeps its spot slice in tiles
//                      of 64.  The tile is v_mfma_f32_16x16x4_f32 with the spots as rows (as pass B of poisson.hip): a
//                      lane holds 16 spots of ONE gene, so the five per-gene sums (deviance, y, y log y, y log V, mu) stay
//                      in its registers for the whole sweep and y arrives as four 16-byte loads of one row.  The per-spot
//                      sums of a tile go across the 16 gene lanes (a halving exchange), then across the 4 waves through
//                      LDS, into one slab per 64-gene block.  The next tile's operands are requested before the current
//                      one is computed.  y is read exactly once.
//   dv_finish_kernel   per gene: the slices' slabs in order, the null deviance; per-workgroup partials of the scalars
//   dv_spot_sum_kernel per spot: the gene blocks' slabs in order
//   dv_total_kernel    the scalars from the partials (one workgroup)
//
// Sparse (gpz_poisson_deviance_sparse): where y = 0 the unit deviance is 2 mu and sum mu factorises,
//   sum_n mu[d,n] = sum_l W[d,l] a[l],  a[l] = sum_n V[n] m[l,n];   sum_d mu[d,n] = V[n] sum_l c[l] m[l,n],  c[l] = sum_d W[d,l]
// so every output is that dense term plus a sum over the stored values of 2 (y log(y / mu) - y).  The layout, the batch
// view (idx / pos) and the work split are those of poisson_sparse.hip: one wave per batch spot, one wave per chunk of at
// most 512 consecutive non-zeros of a gene row.  The gene pass forms mu again at each non-zero; the workspace holds
// nothing of nnz elements (the chunk list has D + nnz / 512 entries).
#include "common.h"
#include "mmops.h"
#include "sparse_rows.h"

namespace gpz {

constexpr int DVMAXL = 64;        // factors
constexpr int DV_TS = 64;         // spots per tile
constexpr int DV_TG = 16;         // genes per wave tile
constexpr int DV_BG = 64;         // genes per workgroup (4 waves): one per-spot slab each
constexpr int DV_Q = 5;           // per-gene sums: deviance, y, y log y, y log V, mu
constexpr int DV_CHUNK = 512;     // sparse: non-zeros of one gene row per wave
constexpr int DV_ROWS = 256;      // rows per workgroup of dv_colsum_kernel
constexpr float DV_LN2 = 0.69314718055994530942f;

typedef float dvf4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ dvf4 dv_mfma(float a, float b, dvf4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// log1p(x), x >= 0, compensated for the rounding of 1 + x (log1p_c of nb_deviance.hip): u = 1 + x, log(u) + (x - (u - 1)) / u;
// below 2^-12 the series x - x^2 / 2 + x^3 / 3.
__device__ __forceinline__ float dv_log1p(float x) {
  const float u = 1.f + x;
  const float big = __builtin_fmaf(DV_LN2, __builtin_amdgcn_logf(u), (x - (u - 1.f)) * __builtin_amdgcn_rcpf(u));
  const float small = x * __builtin_fmaf(x, __builtin_fmaf(x, 1.f / 3.f, -0.5f), 1.f);
  return x < 0x1p-12f ? small : big;
}

// y log(y / mu), y > 0, as a log1p of a non-negative argument on either side of y = mu:
//   y >= mu:  y log1p((y - mu) / mu),      y < mu:  -y log1p((mu - y) / y).
// The difference of two logarithms loses what the deviance is made of where a large count lies next to its rate: at
// y ~ mu ~ 1e4 the unit deviance is about 1 while y log y ~ 1e5 is rounded to 0.008, and log2 y - log2 mu carries the
// absolute error of both logarithms.  y - mu is exact there, so this form keeps the relative error of one log1p.
__device__ __forceinline__ float dv_ylog_ratio(float y, float mu) {
  const bool up = y >= mu;
  const float l = dv_log1p(fabsf(y - mu) * __builtin_amdgcn_rcpf(up ? mu : y));
  return up ? y * l : -y * l;
}

// The same for a stored count of the sparse entry, with the rate in fp64.  There sum mu over ALL (d, n) enters in fp64
// through the factorisation and a stored count adds 2 (y log(y / mu) - y), which is -2 mu to first order: the two meet
// only if the stored term sees the rate the factorisation sums, so the dot product and y - mu are formed in fp64 (an
// fp32 dot product is off by an ulp of mu, 1e-3 at mu = 1e4, per stored count); the logarithm stays fp32.
__device__ __forceinline__ float dv_ylog_ratio(float y, double mu) {
  const bool up = (double)y >= mu;
  const float l = dv_log1p((float)fabs((double)y - mu) * __builtin_amdgcn_rcpf(up ? (float)mu : y));
  return up ? y * l : -y * l;
}

// The element-wise part: 2 (y log(y / mu) - (y - mu)), the difference y - mu formed first (y log(y / mu) is y - mu to first
// order, and either is small beside y); y ln2 log2 y serves the null model's y log y.
struct DvTerm { float dev, yly; };
__device__ __forceinline__ DvTerm dv_term(float y, float mu) {
  const bool pos = y > 0.f;
  const float l2y = __builtin_amdgcn_logf(pos ? y : 1.f), yl = y * DV_LN2;
  const float t = pos ? dv_ylog_ratio(pos ? y : 1.f, mu) : 0.f;
  return DvTerm{2.f * (t - (y - mu)), yl * l2y};
}

// ---------------------------------------------------------------------------------------------------------------------
// dense
// ---------------------------------------------------------------------------------------------------------------------

struct DevArgs {
  const float *mean, *scale, *W, *V, *y;
  float *mF, *Vw, *lV;            // (Lt, N); [Np], [Np] with Np = N rounded up to whole tiles (V = 1 beyond N)
  double* vsum;                   // [1]
  double* gslab;                  // [SN][DV_Q][D]
  float* sslab;                   // [GB][N]
  double* partial;                // [ceil(D / 256)][4]
  double *per_gene, *per_spot, *null_per_gene, *scalars;
  int64_t N, D, Np;
  int Lt, SN, GB, lognormal;
};

__global__ __launch_bounds__(256) void dv_factors_kernel(DevArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (int64_t)a.Lt * a.N) {
    const float s = a.scale[i];
    a.mF[i] = expf(a.mean[i] + (a.lognormal ? 0.5f * s * s : 0.f));
  }
  if (i < a.Np) {
    const float v = i < a.N ? a.V[i] : 1.f;
    a.Vw[i] = v;
    a.lV[i] = logf(v);
  }
}

__global__ __launch_bounds__(256) void dv_vsum_kernel(const float* V, int64_t n, double* out) {
  __shared__ double sh[8];
  double v = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) v += (double)V[i];
  const double t = block_sum(v, sh);
  if (threadIdx.x == 0) out[0] = t;
}

template <int KS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 4))) void dv_tile_kernel(DevArgs a) {
  constexpr bool PFA = KS <= 8;                 // the A operand of the next tile fits in registers beside the current one
  __shared__ float sp[2][4][DV_TS];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int64_t d0 = ((int64_t)blockIdx.x * 4 + wave) * DV_TG;
  const int64_t dcol = d0 + r;                  // this lane's gene (a column of the tile)
  const bool dok = dcol < a.D;
  const int64_t ntiles = (a.N + DV_TS - 1) / DV_TS, tper = (ntiles + a.SN - 1) / a.SN;
  const int64_t t_lo = blockIdx.y * tper, t_hi = (t_lo + tper < ntiles) ? t_lo + tper : ntiles;
  const bool vec = (a.N & 3) == 0 && (reinterpret_cast<uintptr_t>(a.y) & 15) == 0;   // rows of y start 16-byte aligned
  float wb[KS];                                 // B[k = factor 4 ks + q][column = gene r]
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int l = 4 * ks + q;
    wb[ks] = (dok && l < a.Lt) ? a.W[dcol * a.Lt + l] : 0.f;
  }
  const int arow = 16 * (r >> 2) + (r & 3);     // A row r of sub-tile c is spot 16 (r >> 2) + 4c + (r & 3) of the tile
  double gsum[DV_Q];
#pragma unroll
  for (int k = 0; k < DV_Q; ++k) gsum[k] = 0.0;
  // One tile's operands: y (four 16-byte loads of the lane's gene row), V and log V of its 16 spots, and the A operand of the
  // rate product, m[factor 4 ks + q][spot arow + 4c].  The next tile's are requested before the current one is computed:
  // the loop is otherwise bound by the latency of these reads.
  struct Tile { dvf4 yv[4], vv[4], lv[4]; float av[4][KS]; };
  auto load_tile = [&](int64_t tt, Tile& T) __attribute__((always_inline)) {
    const int64_t n0 = tt * DV_TS;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int64_t n = n0 + 16 * q + 4 * c;    // < Np: the padded arrays cover the tile
      T.vv[c] = *reinterpret_cast<const dvf4*>(a.Vw + n);
      T.lv[c] = *reinterpret_cast<const dvf4*>(a.lV + n);
      T.yv[c] = dvf4{0, 0, 0, 0};
      if (dok) {
        const float* yp = a.y + dcol * a.N + n;
        if (vec && n + 3 < a.N) T.yv[c] = *reinterpret_cast<const dvf4*>(yp);
        else {
#pragma unroll
          for (int g = 0; g < 4; ++g) if (n + g < a.N) T.yv[c][g] = yp[g];
        }
      }
    }
  };
  auto load_a = [&](int64_t tt, Tile& T) __attribute__((always_inline)) {
    const int64_t n0 = tt * DV_TS;
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
  const bool b8 = (r & 8) != 0, b4 = (r & 4) != 0, b2 = (r & 2) != 0, b1 = (r & 1) != 0;
  int par = 0;
  for (int64_t tt = t_lo; tt < t_hi; ++tt, par ^= 1) {
    const int64_t n0 = tt * DV_TS;
    if (!PFA) load_a(tt, cur);
    if (tt + 1 < t_hi) { load_tile(tt + 1, nxt); if (PFA) load_a(tt + 1, nxt); }
    // rate tile: row 4q + g of sub-tile c is spot 16q + 4c + g, column r is gene d0 + r
    dvf4 z[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      z[c] = dvf4{0, 0, 0, 0};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) z[c] = dv_mfma(cur.av[c][ks], wb[ks], z[c]);
    }
    float f[DV_Q] = {0.f, 0.f, 0.f, 0.f, 0.f};
    float v[16];                                // v[4c + g]: the unit deviance at spot 16q + 4c + g of gene d0 + r
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const bool ok = dok && n0 + 16 * q + 4 * c + g < a.N;
        const float y1 = cur.yv[c][g];          // 0 where the element does not exist
        const float mu = ok ? cur.vv[c][g] * z[c][g] : 1.f;
        const DvTerm t = dv_term(y1, mu);
        const float dev = ok ? t.dev : 0.f;
        f[0] += dev; f[1] += y1; f[2] += t.yly; f[3] += y1 * cur.lv[c][g]; f[4] += ok ? mu : 0.f;
        v[4 * c + g] = dev;
      }
#pragma unroll
    for (int k = 0; k < DV_Q; ++k) gsum[k] += (double)f[k];
    // The spots' sums over this wave's 16 genes: a halving exchange across the gene lanes r -- at each step a lane keeps the
    // half of its values whose index has its own bit of r and adds the partner's copy of them -- leaves lane r with the
    // sum over all 16 genes of value r, i.e. of spot 16q + r = the lane's own number in the wave.  One fixed tree per spot.
#pragma unroll
    for (int i = 0; i < 8; ++i) { const float keep = b8 ? v[i + 8] : v[i], send = b8 ? v[i] : v[i + 8]; v[i] = keep + __shfl_xor(send, 8); }
#pragma unroll
    for (int i = 0; i < 4; ++i) { const float keep = b4 ? v[i + 4] : v[i], send = b4 ? v[i] : v[i + 4]; v[i] = keep + __shfl_xor(send, 4); }
#pragma unroll
    for (int i = 0; i < 2; ++i) { const float keep = b2 ? v[i + 2] : v[i], send = b2 ? v[i] : v[i + 2]; v[i] = keep + __shfl_xor(send, 2); }
    { const float keep = b1 ? v[1] : v[0], send = b1 ? v[0] : v[1]; v[0] = keep + __shfl_xor(send, 1); }
    sp[par][wave][lane] = v[0];
    // One barrier per tile: the buffer written two tiles ago was read before its readers reached this one.
    __syncthreads();
    if (threadIdx.x < DV_TS && n0 + threadIdx.x < a.N)
      a.sslab[(int64_t)blockIdx.x * a.N + n0 + threadIdx.x] =
          (sp[par][0][threadIdx.x] + sp[par][1][threadIdx.x]) + (sp[par][2][threadIdx.x] + sp[par][3][threadIdx.x]);
    cur = nxt;
  }
  // the gene's sums over this slice: the four spot groups q in a fixed order, lanes q == 0 write
#pragma unroll
  for (int k = 0; k < DV_Q; ++k) {
    double v = gsum[k];
    v += __shfl_xor(v, 16); v += __shfl_xor(v, 32);
    if (q == 0 && dok) a.gslab[((int64_t)blockIdx.y * DV_Q + k) * a.D + dcol] = v;
  }
}

// per_gene, null_per_gene and the workgroup's partials of {total, sum y, sum mu, null total}; gslab [SN][DV_Q][D]
__global__ __launch_bounds__(256) void dv_finish_kernel(const double* gslab, int SN, int64_t D, const double* vsum,
                                                        double* per_gene, double* null_per_gene, double* partial) {
  __shared__ double sh[8];
  const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double g[DV_Q] = {0.0, 0.0, 0.0, 0.0, 0.0}, nul = 0.0;
  if (d < D) {
    for (int s = 0; s < SN; ++s)
#pragma unroll
      for (int k = 0; k < DV_Q; ++k) g[k] += gslab[((int64_t)s * DV_Q + k) * D + d];
    if (g[1] > 0.0) nul = 2.0 * (g[2] - g[3] - g[1] * log(g[1] / vsum[0]));
    per_gene[d] = g[0];
    null_per_gene[d] = nul;
  }
  const double t0 = block_sum(g[0], sh), t1 = block_sum(g[1], sh), t2 = block_sum(g[4], sh), t3 = block_sum(nul, sh);
  if (threadIdx.x == 0) {
    double* p = partial + (int64_t)blockIdx.x * 4;
    p[0] = t0; p[1] = t1; p[2] = t2; p[3] = t3;
  }
}

__global__ __launch_bounds__(256) void dv_total_kernel(const double* partial, int64_t nb, double* scalars) {
  __shared__ double sh[8];
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t b = threadIdx.x; b < nb; b += 256)
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] += partial[b * 4 + k];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double t = block_sum(v[k], sh);
    if (threadIdx.x == 0) scalars[k] = t;
  }
}

__global__ __launch_bounds__(256) void dv_spot_sum_kernel(const float* sslab, int GB, int64_t N, double* per_spot) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  double v = 0.0;
#pragma unroll 4
  for (int b = 0; b < GB; ++b) v += (double)sslab[(int64_t)b * N + n];
  per_spot[n] = v;
}

static int dv_ksteps(int Lt) {                  // the instances of poisson.hip: k-steps of 4 factors
  const int k = (Lt + 3) / 4;
  return k <= 10 ? k : k <= 12 ? 12 : k <= 14 ? 14 : 16;
}

struct DevPlan { int SN, GB, KS; int64_t tper, Np, nbD; size_t bytes; };

static DevPlan dev_plan(int64_t N, int64_t D, int Lt, DevArgs* a, void* ws) {
  DevPlan p;
  const int64_t ntiles = (N + DV_TS - 1) / DV_TS;
  p.GB = (int)((D + DV_BG - 1) / DV_BG);
  // enough (gene block, spot slice) workgroups to fill the device a few times over, slices of at least 8 tiles
  int64_t SN = (1024 + p.GB - 1) / p.GB;
  if (SN > (N + 511) / 512) SN = (N + 511) / 512;
  if (SN > 16) SN = 16;
  if (SN < 1) SN = 1;
  p.SN = (int)SN;
  p.tper = (ntiles + SN - 1) / SN;
  p.Np = ntiles * DV_TS;
  p.KS = dv_ksteps(Lt);
  p.nbD = (D + 255) / 256;
  Carver c(ws);
  float* mF = c.take<float>((size_t)Lt * N);
  float* Vw = c.take<float>((size_t)p.Np);
  float* lV = c.take<float>((size_t)p.Np);
  double* vsum = c.take<double>(1);
  double* gslab = c.take<double>((size_t)p.SN * DV_Q * D);
  float* sslab = c.take<float>((size_t)p.GB * N);
  double* partial = c.take<double>((size_t)p.nbD * 4);
  p.bytes = c.used();
  if (a) {
    a->mF = mF; a->Vw = Vw; a->lV = lV; a->vsum = vsum; a->gslab = gslab; a->sslab = sslab; a->partial = partial;
    a->SN = p.SN; a->GB = p.GB; a->Np = p.Np;
  }
  return p;
}

static int dev_check_shape(const char* who, int64_t N, int64_t D, int Lt) {
  GPZ_REQUIRE(N >= 1 && D >= 1, "%s: bad extents (N = %lld, D = %lld)", who, (long long)N, (long long)D);
  GPZ_REQUIRE(Lt >= 1 && Lt <= DVMAXL, "%s: %d factors unsupported (1..%d)", who, Lt, DVMAXL);
  GPZ_REQUIRE(N < (1ll << 31) && D < (1ll << 31), "%s: spots and genes are indexed with 32 bits", who);
  return 0;
}

template <int KS>
static void dev_launch_tiles(const DevArgs& a, hipStream_t s) {
  hipLaunchKernelGGL((dv_tile_kernel<KS>), dim3((unsigned)a.GB, (unsigned)a.SN), dim3(256), 0, s, a);
}

// ---------------------------------------------------------------------------------------------------------------------
// sparse
// ---------------------------------------------------------------------------------------------------------------------

struct DevSpArgs {
  const float *mean, *scale, *W, *V;
  const int64_t* col_ptr; const int32_t* col_gene; const float* col_val;
  const int64_t* row_ptr; const int32_t* row_spot; const int32_t* row_perm;
  const int32_t *idx, *pos;
  float *mT, *lV;                 // [B][LT] (zeros beyond Lt), [B]
  double *cpart, *apart;          // [nbW][LT], [nbS][LT]
  double *cD, *aD, *vsum;         // [64]: c[l] = sum_d W[d,l];  [64]: a[l] = sum_n V[n] m[l,n];  [1]
  int32_t *cstart, *chunk_gene;   // [D + 1], [nchunks]
  double* part;                   // [nchunks][4]: sums over the chunk of 2 (y log(y / mu) - y), y, y log y, y log V
  double* gq;                     // [DV_Q][D]
  double* partial;                // [ceil(D / 256)][4]
  double *per_gene, *per_spot, *null_per_gene, *scalars;
  int64_t N, B, D, nnz, nchunks;
  int Lt, LT, nbW, nbS, lognormal;
};

static int dv_instance(int Lt) {
  const int sizes[] = {4, 8, 12, 16, 20, 24, 32, 40, 48, 64};
  for (int s : sizes) if (Lt <= s) return s;
  return 0;
}

__global__ __launch_bounds__(256) void dv_sp_factors_kernel(DevSpArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < a.B * a.LT) {
    const int64_t j = i / a.LT;
    const int l = (int)(i - j * a.LT);
    float m = 0.f;
    if (l < a.Lt) {
      const float s = a.scale[(int64_t)l * a.B + j];
      m = expf(a.mean[(int64_t)l * a.B + j] + (a.lognormal ? 0.5f * s * s : 0.f));
    }
    a.mT[i] = m;
  }
  if (i < a.B) a.lV[i] = logf(a.V[i]);
}

// part[b][l] = sum over rows b * 256 ... of rowscale[row] src[row * stride + l] (rowscale nullable: 1; l < ncols, zero
// beyond), in fp64 and a fixed order
__global__ __launch_bounds__(256) void dv_colsum_kernel(const float* src, const float* rowscale, int64_t R, int stride,
                                                        int ncols, int LT, double* part) {
  __shared__ double sh[4][64];
  const int l = threadIdx.x & 63, r = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * DV_ROWS, r1 = r0 + DV_ROWS < R ? r0 + DV_ROWS : R;
  double v = 0.0;
  if (l < ncols) {
    for (int64_t row = r0 + r; row < r1; row += 4)
      v += (double)src[row * stride + l] * (rowscale ? (double)rowscale[row] : 1.0);
  }
  sh[r][l] = v;
  __syncthreads();
  if (r == 0 && l < LT) part[(int64_t)blockIdx.x * LT + l] = (sh[0][l] + sh[1][l]) + (sh[2][l] + sh[3][l]);
}

// out[l] = sum_b part[b][l] in ascending b (one workgroup of 64 threads); zeros from LT to 63
__global__ __launch_bounds__(64) void dv_colsum_final_kernel(const double* part, int nb, int LT, double* out) {
  const int l = threadIdx.x;
  double v = 0.0;
  if (l < LT)
    for (int b = 0; b < nb; ++b) v += part[(int64_t)b * LT + l];
  out[l] = v;
}

// Spot pass.  4 waves per workgroup, wave = batch spot j (global spot n = idx[j]); lanes stride over the column's
// non-zeros.  per_spot[j] = 2 V[j] sum_l c[l] m[l,j] + sum over the column of 2 (y log(y / mu) - y).  No barrier.
template <int LT>
__global__ __launch_bounds__(256) void dv_sp_spot_kernel(DevSpArgs a) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t j = (int64_t)blockIdx.x * 4 + wave;
  if (j >= a.B) return;
  const int64_t n = a.idx ? a.idx[j] : j;
  const int64_t k0 = a.col_ptr[n], k1 = a.col_ptr[n + 1];
  const float vn = a.V[j];
  float m[LT];
  const dvf4* mp = reinterpret_cast<const dvf4*>(a.mT + j * LT);
#pragma unroll
  for (int l = 0; l < LT; l += 4) {
    const dvf4 v = mp[l / 4];
    m[l] = v[0]; m[l + 1] = v[1]; m[l + 2] = v[2]; m[l + 3] = v[3];
  }
  double acc = 0.0;
  for (int64_t k = k0 + lane; k < k1; k += 64) {
    const float y = a.col_val[k];
    if (y == 0.f) continue;                 // an explicit zero: 0 log(.) is never formed
    float w[LT];
    load_w<LT>(a.W, a.col_gene[k], a.Lt, w);
    double z = 0.0;
#pragma unroll
    for (int l = 0; l < LT; ++l) z = __builtin_fma((double)w[l], (double)m[l], z);
    acc += 2.0 * ((double)dv_ylog_ratio(y, (double)vn * z) - (double)y);
  }
  acc = wave_sum(acc);
  const double cm = wave_sum(lane < LT ? a.cD[lane] * (double)a.mT[j * LT + lane] : 0.0);
  if (lane == 0) a.per_spot[j] = 2.0 * (double)vn * cm + acc;
}

// Gene pass.  4 waves per workgroup, wave = chunk w of the work list: at most 512 consecutive non-zeros of one gene row.
// The wave packs the chunk's entries that lie in the batch (pos[n] >= 0) and are not stored zeros into LDS, in their
// order, then every lane takes every 64th packed entry.
template <int LT>
__global__ __launch_bounds__(256) void dv_sp_gene_kernel(DevSpArgs a) {
  __shared__ int32_t lj[4][DV_CHUNK];
  __shared__ float ly[4][DV_CHUNK];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t wi = (int64_t)blockIdx.x * 4 + wave;
  const int g = wi < a.nchunks ? a.chunk_gene[wi] : -1;
  int cnt = 0;
  if (g >= 0) {
    const int64_t p0 = a.row_ptr[g] + (wi - a.cstart[g]) * DV_CHUNK;
    const int64_t pe = a.row_ptr[g + 1], p1 = p0 + DV_CHUNK < pe ? p0 + DV_CHUNK : pe;
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
  float acc[4] = {0.f, 0.f, 0.f, 0.f};           // at most 8 entries per lane
  double ys = 0.0;                               // sum y, exact: it meets sum y log(y / mu) below
  for (int i = lane; i < cnt; i += 64) {
    const int64_t j = lj[wave][i];
    const float y = ly[wave][i];
    const dvf4* mp = reinterpret_cast<const dvf4*>(a.mT + j * LT);
    double z = 0.0;
#pragma unroll
    for (int l = 0; l < LT; l += 4) {
      const dvf4 v = mp[l / 4];
#pragma unroll
      for (int i = 0; i < 4; ++i) z = __builtin_fma((double)w[l + i], (double)v[i], z);
    }
    const float l2y = __builtin_amdgcn_logf(y), yl = y * DV_LN2;
    acc[0] += dv_ylog_ratio(y, (double)a.V[j] * z);
    ys += (double)y;
    acc[2] += yl * l2y;
    acc[3] += y * a.lV[j];
  }
  // part[0] = sum 2 (y log(y / mu) - y): the two sums meet in fp64 (y log(y / mu) is small beside y next to y = mu)
  double t[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) t[k] = wave_sum(k == 1 ? ys : (double)acc[k]);
  t[0] = 2.0 * (t[0] - t[1]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) a.part[wi * 4 + k] = t[k];
  }
}

// gq[.][d] from the row's chunk partials in chunk order and the dense term sum_l W[d,l] a[l]
__global__ __launch_bounds__(256) void dv_sp_gene_finish_kernel(DevSpArgs a) {
  __shared__ double sa[64];
  if (threadIdx.x < 64) sa[threadIdx.x] = a.aD[threadIdx.x];
  __syncthreads();
  const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (d >= a.D) return;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t c = a.cstart[d]; c < a.cstart[d + 1]; ++c)
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] += a.part[c * 4 + k];
  double smu = 0.0;
  for (int l = 0; l < a.Lt; ++l) smu += (double)a.W[d * a.Lt + l] * sa[l];
  a.gq[d] = 2.0 * smu + v[0];
  a.gq[a.D + d] = v[1];
  a.gq[2 * a.D + d] = v[2];
  a.gq[3 * a.D + d] = v[3];
  a.gq[4 * a.D + d] = smu;
}

struct DevSpPlan { int LT, nbW, nbS; int64_t nchunks, nbD; size_t bytes; };

static DevSpPlan dev_sp_plan(int64_t B, int64_t D, int Lt, int64_t nnz, DevSpArgs* a, void* ws) {
  DevSpPlan p;
  p.LT = dv_instance(Lt);
  p.nbW = (int)((D + DV_ROWS - 1) / DV_ROWS);
  p.nbS = (int)((B + DV_ROWS - 1) / DV_ROWS);
  p.nchunks = D + nnz / DV_CHUNK;            // sum_d ceil(len_d / C) <= D + floor(nnz / C)
  p.nbD = (D + 255) / 256;
  Carver c(ws);
  float* mT = c.take<float>((size_t)B * p.LT);
  float* lV = c.take<float>((size_t)B);
  double* cpart = c.take<double>((size_t)p.nbW * p.LT);
  double* apart = c.take<double>((size_t)p.nbS * p.LT);
  double* cD = c.take<double>(64);
  double* aD = c.take<double>(64);
  double* vsum = c.take<double>(1);
  int32_t* cstart = c.take<int32_t>((size_t)D + 1);
  int32_t* chunk_gene = c.take<int32_t>((size_t)p.nchunks);
  double* part = c.take<double>((size_t)p.nchunks * 4);
  double* gq = c.take<double>((size_t)DV_Q * D);
  double* partial = c.take<double>((size_t)p.nbD * 4);
  p.bytes = c.used();
  if (a) {
    a->mT = mT; a->lV = lV; a->cpart = cpart; a->apart = apart; a->cD = cD; a->aD = aD; a->vsum = vsum; a->cstart = cstart;
    a->chunk_gene = chunk_gene; a->part = part; a->gq = gq; a->partial = partial;
    a->LT = p.LT; a->nbW = p.nbW; a->nbS = p.nbS; a->nchunks = p.nchunks;
  }
  return p;
}

static int dev_sp_check_shape(const char* who, int64_t N, int64_t B, int64_t D, int Lt, int64_t nnz) {
  GPZ_REQUIRE(N >= 1 && B >= 1 && D >= 1 && nnz >= 0, "%s: bad extents (N = %lld, B = %lld, D = %lld, nnz = %lld)", who,
              (long long)N, (long long)B, (long long)D, (long long)nnz);
  GPZ_REQUIRE(B <= N, "%s: a batch of %lld distinct spots out of %lld", who, (long long)B, (long long)N);
  GPZ_REQUIRE(Lt >= 1 && Lt <= DVMAXL, "%s: %d factors unsupported (1..%d)", who, Lt, DVMAXL);
  GPZ_REQUIRE(N < (1ll << 31) && D < (1ll << 31) && nnz < (1ll << 31) && D + nnz / DV_CHUNK < (1ll << 31),
              "%s: spots, genes and non-zeros are indexed with 32 bits", who);
  return 0;
}

template <int LT>
static int dev_sp_passes(const DevSpArgs& a, hipStream_t s) {
  hipLaunchKernelGGL((dv_sp_spot_kernel<LT>), dim3((unsigned)((a.B + 3) / 4)), dim3(256), 0, s, a);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL((dv_sp_gene_kernel<LT>), dim3((unsigned)((a.nchunks + 3) / 4)), dim3(256), 0, s, a);
  GPZ_LAUNCH_OK();
  return 0;
}

}  // namespace gpz

using namespace gpz;

extern "C" int gpz_poisson_deviance_plan(int64_t N, int64_t D, int32_t Lt, int32_t* spots_per_tile, int32_t* genes_per_tile,
                                         int32_t* genes_per_block, int32_t* gene_slices, int32_t* spot_slices,
                                         int64_t* tiles_per_spot_slice, int32_t* factors_padded) {
  if (int rc = dev_check_shape("gpz_poisson_deviance_plan", N, D, Lt)) return rc;
  const DevPlan p = dev_plan(N, D, Lt, nullptr, nullptr);
  if (spots_per_tile) *spots_per_tile = DV_TS;
  if (genes_per_tile) *genes_per_tile = DV_TG;
  if (genes_per_block) *genes_per_block = DV_BG;
  if (gene_slices) *gene_slices = p.GB;
  if (spot_slices) *spot_slices = p.SN;
  if (tiles_per_spot_slice) *tiles_per_spot_slice = p.tper;
  if (factors_padded) *factors_padded = 4 * p.KS;
  return 0;
}

extern "C" size_t gpz_poisson_deviance_workspace_bytes(int64_t N, int64_t D, int32_t Lt) {
  if (dev_check_shape("gpz_poisson_deviance_workspace_bytes", N, D, Lt)) return 0;
  return dev_plan(N, D, Lt, nullptr, nullptr).bytes;
}

extern "C" int gpz_poisson_deviance(const float* mean, const float* scale, const float* W, const float* V, const float* y,
                                    int64_t N, int64_t D, int32_t Lt, int32_t lognormal_mean, double* per_gene,
                                    double* per_spot, double* null_per_gene, double* scalars, void* ws, size_t ws_bytes,
                                    void* stream) {
  if (int rc = dev_check_shape("gpz_poisson_deviance", N, D, Lt)) return rc;
  GPZ_REQUIRE(mean && scale && W && V && y && per_gene && per_spot && null_per_gene && scalars && ws,
              "gpz_poisson_deviance: null pointer");
  GPZ_REQUIRE(((reinterpret_cast<uintptr_t>(W) | reinterpret_cast<uintptr_t>(ws)) & 15) == 0,
              "gpz_poisson_deviance: W and the workspace must be 16-byte aligned");
  DevArgs a;
  const DevPlan p = dev_plan(N, D, Lt, &a, ws);
  GPZ_REQUIRE(ws_bytes >= p.bytes, "gpz_poisson_deviance: workspace of %zu bytes, %zu needed", ws_bytes, p.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  a.mean = mean; a.scale = scale; a.W = W; a.V = V; a.y = y;
  a.per_gene = per_gene; a.per_spot = per_spot; a.null_per_gene = null_per_gene; a.scalars = scalars;
  a.N = N; a.D = D; a.Lt = Lt; a.lognormal = lognormal_mean != 0;
  const int64_t tot = (int64_t)Lt * N > a.Np ? (int64_t)Lt * N : a.Np;
  hipLaunchKernelGGL(dv_factors_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, a);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(dv_vsum_kernel, dim3(1), dim3(256), 0, s, V, N, a.vsum);
  GPZ_LAUNCH_OK();
  switch (p.KS) {
    case 1: dev_launch_tiles<1>(a, s); break;
    case 2: dev_launch_tiles<2>(a, s); break;
    case 3: dev_launch_tiles<3>(a, s); break;
    case 4: dev_launch_tiles<4>(a, s); break;
    case 5: dev_launch_tiles<5>(a, s); break;
    case 6: dev_launch_tiles<6>(a, s); break;
    case 7: dev_launch_tiles<7>(a, s); break;
    case 8: dev_launch_tiles<8>(a, s); break;
    case 9: dev_launch_tiles<9>(a, s); break;
    case 10: dev_launch_tiles<10>(a, s); break;
    case 12: dev_launch_tiles<12>(a, s); break;
    case 14: dev_launch_tiles<14>(a, s); break;
    default: dev_launch_tiles<16>(a, s); break;
  }
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(dv_finish_kernel, dim3((unsigned)p.nbD), dim3(256), 0, s, a.gslab, a.SN, D, a.vsum, per_gene,
                     null_per_gene, a.partial);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(dv_spot_sum_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, a.sslab, a.GB, N, per_spot);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(dv_total_kernel, dim3(1), dim3(256), 0, s, a.partial, p.nbD, scalars);
  GPZ_LAUNCH_OK();
  return 0;
}

extern "C" int gpz_poisson_deviance_sparse_plan(int64_t N, int64_t B, int64_t D, int32_t Lt, int64_t nnz, int32_t* gene_chunk,
                                                int32_t* spot_chunk, int64_t* n_gene_chunks, int32_t* factors_padded) {
  if (int rc = dev_sp_check_shape("gpz_poisson_deviance_sparse_plan", N, B, D, Lt, nnz)) return rc;
  const DevSpPlan p = dev_sp_plan(B, D, Lt, nnz, nullptr, nullptr);
  if (gene_chunk) *gene_chunk = DV_CHUNK;
  if (spot_chunk) *spot_chunk = 0;
  if (n_gene_chunks) *n_gene_chunks = p.nchunks;
  if (factors_padded) *factors_padded = p.LT;
  return 0;
}

extern "C" size_t gpz_poisson_deviance_sparse_workspace_bytes(int64_t N, int64_t B, int64_t D, int64_t nnz, int32_t Lt) {
  if (dev_sp_check_shape("gpz_poisson_deviance_sparse_workspace_bytes", N, B, D, Lt, nnz)) return 0;
  return dev_sp_plan(B, D, Lt, nnz, nullptr, nullptr).bytes;
}

extern "C" int gpz_poisson_deviance_sparse(const float* mean, const float* scale, const float* W, const float* V,
                                           const int64_t* col_ptr, const int32_t* col_gene, const float* col_val,
                                           const int64_t* row_ptr, const int32_t* row_spot, const int32_t* row_perm,
                                           const int32_t* idx, const int32_t* pos, int64_t N, int64_t B, int64_t D,
                                           int64_t nnz, int32_t Lt, int32_t lognormal_mean, double* per_gene,
                                           double* per_spot, double* null_per_gene, double* scalars, void* ws,
                                           size_t ws_bytes, void* stream) {
  if (int rc = dev_sp_check_shape("gpz_poisson_deviance_sparse", N, B, D, Lt, nnz)) return rc;
  GPZ_REQUIRE(mean && scale && W && V && col_ptr && row_ptr && per_gene && per_spot && null_per_gene && scalars && ws,
              "gpz_poisson_deviance_sparse: null pointer");
  GPZ_REQUIRE(nnz == 0 || (col_gene && col_val && row_spot && row_perm), "gpz_poisson_deviance_sparse: null pointer (non-zeros)");
  GPZ_REQUIRE((idx == nullptr) == (pos == nullptr), "gpz_poisson_deviance_sparse: idx and pos come together (both null: all spots)");
  GPZ_REQUIRE(idx || B == N, "gpz_poisson_deviance_sparse: B = %lld of N = %lld spots needs idx and pos", (long long)B,
              (long long)N);
  GPZ_REQUIRE(((reinterpret_cast<uintptr_t>(W) | reinterpret_cast<uintptr_t>(ws)) & 15) == 0,
              "gpz_poisson_deviance_sparse: W and the workspace must be 16-byte aligned");
  DevSpArgs a;
  const DevSpPlan p = dev_sp_plan(B, D, Lt, nnz, &a, ws);
  GPZ_REQUIRE(ws_bytes >= p.bytes, "gpz_poisson_deviance_sparse: workspace of %zu bytes, %zu needed", ws_bytes, p.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  a.mean = mean; a.scale = scale; a.W = W; a.V = V;
  a.col_ptr = col_ptr; a.col_gene = col_gene; a.col_val = col_val;
  a.row_ptr = row_ptr; a.row_spot = row_spot; a.row_perm = row_perm; a.idx = idx; a.pos = pos;
  a.per_gene = per_gene; a.per_spot = per_spot; a.null_per_gene = null_per_gene; a.scalars = scalars;
  a.N = N; a.B = B; a.D = D; a.nnz = nnz; a.Lt = Lt; a.lognormal = lognormal_mean != 0;
  hipLaunchKernelGGL(dv_sp_factors_kernel, dim3((unsigned)((B * a.LT + 255) / 256)), dim3(256), 0, s, a);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(dv_vsum_kernel, dim3(1), dim3(256), 0, s, V, B, a.vsum);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(dv_colsum_kernel, dim3((unsigned)a.nbW), dim3(256), 0, s, W, (const float*)nullptr, D, (int)Lt, (int)Lt,
                     a.LT, a.cpart);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(dv_colsum_final_kernel, dim3(1), dim3(64), 0, s, a.cpart, a.nbW, a.LT, a.cD);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(dv_colsum_kernel, dim3((unsigned)a.nbS), dim3(256), 0, s, a.mT, V, B, a.LT, a.LT, a.LT, a.apart);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(dv_colsum_final_kernel, dim3(1), dim3(64), 0, s, a.apart, a.nbS, a.LT, a.aD);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(chunks_kernel, dim3(1), dim3(1024), 0, s, a.row_ptr, a.D, a.nchunks, DV_CHUNK, false, a.cstart, a.chunk_gene);
  GPZ_LAUNCH_OK();
  int rc;
  switch (a.LT) {
    case 4: rc = dev_sp_passes<4>(a, s); break;
    case 8: rc = dev_sp_passes<8>(a, s); break;
    case 12: rc = dev_sp_passes<12>(a, s); break;
    case 16: rc = dev_sp_passes<16>(a, s); break;
    case 20: rc = dev_sp_passes<20>(a, s); break;
    case 24: rc = dev_sp_passes<24>(a, s); break;
    case 32: rc = dev_sp_passes<32>(a, s); break;
    case 40: rc = dev_sp_passes<40>(a, s); break;
    case 48: rc = dev_sp_passes<48>(a, s); break;
    default: rc = dev_sp_passes<64>(a, s); break;
  }
  if (rc) return rc;
  hipLaunchKernelGGL(dv_sp_gene_finish_kernel, dim3((unsigned)p.nbD), dim3(256), 0, s, a);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(dv_finish_kernel, dim3((unsigned)p.nbD), dim3(256), 0, s, a.gq, 1, D, a.vsum, per_gene, null_per_gene,
                     a.partial);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(dv_total_kernel, dim3(1), dim3(256), 0, s, a.partial, p.nbD, scalars);
  GPZ_LAUNCH_OK();
  return 0;
}
