// gram.hip -- the normal equations of a kernel least-squares fit in ONE pass over the data, K_zx never stored:
//   G[l] = K_zx K_xz + jitter I  (M,M)   and   b[l] = K_zx F[l]^T  (R,M),   K_zx = k_l(Z, X),
// what the reference's notebooks form as `Kzx @ Kxz` and `Kzx @ F` from a materialised kernel(Z, X)
// (Slideseqv2_estimate_lengthscales.ipynb build_model_scracth, NSF_Hybrid_benchmark.ipynb) to start gp.mu.
//
// gram_kernel: a workgroup owns (lower-triangle 128 x 128 tile (ti >= tj), latent, N-split).  Per step of its split
// it generates the covariance panels k(Z_ti-block, x-chunk) and k(Z_tj-block, x-chunk) from the coordinates into LDS
// ([row][column of the chunk], the layout both MFMA operands read) and accumulates panel_i panel_j^T on the matrix
// cores: 8 waves (2 x 4), 64 x 32 outputs per wave in 8 accumulator tiles.  A diagonal tile generates ONE panel, uses it
// as both operands, and multiplies the same panel with the F chunk (R <= 16 or <= 64 rows, one or four more accumulator
// tiles per wave) for its 128 rows of b.  Double buffered: the panels of step t + 1 are generated while step t runs,
// one barrier per step.  Nothing of K_zx reaches memory.
//   fp32: the entries are cov.h's (cov_const / cov_d2 / cov_radial / cov_value: the bits gpz_kfill writes), products
//         and the sums inside a split on v_mfma_f32_16x16x4_f32, 32 columns per step;
//   fp64: kfill.hip's fp64 formulas, v_mfma_f64_16x16x4_f64, 16 columns per step (same template, not tuned).
// Columns beyond the split's end are zeroed through the covariance constants (cov.h, CovConst) and F is read as 0
// there; rows beyond M are generated from zero coordinates and never leave the workgroup's tile (the reduction reads
// only rows < M).  Every global read is guarded by the arrays' extents.
//
// gram_reduce_kernel: adds the splits' partial tiles in ascending split order in fp64, mirrors the lower triangle, adds
// the jitter to the diagonal, writes G and b.  No floating-point atomics, no flags, no ticket: a plain grid plus one
// reduction launch; two calls on the same input agree bit for bit.
//
// Plan (gram_plan, host only): tile 128; a split covers at most 16 384 columns, so an fp32 partial sum has at most
// 16 384 terms (its rounding error grows like sqrt(16 384) 2^-24 = 8e-6 of the sum; the splits are added in fp64), and
// there are at least enough splits for 512 workgroups (two per CU) while a split keeps >= 4 steps.
// Workspace: per split and latent the lower-triangle tiles, nt (nt + 1) / 2 x 128 x 128 values, plus nt x RB x 128 for
// b (nt = ceil(M / 128), RB = 16 or 64), in the compute precision: bytes = splits x n_latent x (nt (nt + 1) / 2 x 16 384
// + nt x RB x 128) x sizeof(T), independent of N for a fixed number of splits, and for M >= 1024 below splits x
// sizeof(G).
#include "common.h"
#include "cov.h"

#include <mutex>
#include <type_traits>

namespace gpz {
namespace {

typedef float g_f32x4 __attribute__((ext_vector_type(4)));
typedef double g_f64x4 __attribute__((ext_vector_type(4)));
typedef double g_f64x2 __attribute__((ext_vector_type(2)));

constexpr int GR_TILE = 128;
constexpr int GR_THREADS = 512;
constexpr int64_t GR_SPLIT_COLS = 16384;   // most columns one fp32 partial sum runs over
constexpr int64_t GR_TARGET_WGS = 512;     // workgroups wanted before N stops being split further
constexpr int GR_MIN_STEPS = 4;            // steps a split keeps at least
constexpr int GR_MAX_R = 64;
constexpr int64_t GR_MAX_M = 8192;

template <typename T> struct GramT;
template <> struct GramT<float> {
  using acc_t = g_f32x4;
  using vec_t = g_f32x4;
  static constexpr int VEC = 4, BK = 32;
  static __device__ __forceinline__ acc_t mma(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ int crow(int q, int g) { return 4 * q + g; }   // C/D: col = lane & 15, row = 4 (lane >> 4) + reg
};
template <> struct GramT<double> {
  using acc_t = g_f64x4;
  using vec_t = g_f64x2;
  static constexpr int VEC = 2, BK = 16;
  static __device__ __forceinline__ acc_t mma(double a, double b, acc_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ int crow(int q, int g) { return q + 4 * g; }   // f64: row = (lane >> 4) + 4 reg
};

// One covariance family in one precision: init() from (sigma, lengthscale), zero() for a padding column, eval().
template <typename T, int KIND> struct GramCov;
template <int KIND> struct GramCov<float, KIND> {
  CovConst c;
  __device__ __forceinline__ void init(float s, float e) { c = cov_const<KIND>(s, e); }
  __device__ __forceinline__ void zero() { c.amp = 0.f; c.c0 = 0.f; c.c2 = 0.f; }
  __device__ __forceinline__ float eval(const float* z, const float* x, bool low_d) const {
    const float d2 = low_d ? cov_d2<2>(z, x) : cov_d2<4>(z, x);    // unused coordinates are 0 on both sides: fma(0, 0, acc) = acc
    return cov_value<KIND>(cov_radial<KIND>(d2), c.amp, c.c0, c.c1, c.c2);
  }
};
template <int KIND> struct GramCov<double, KIND> {      // the fp64 forms of kfill.hip
  double amp, cf;
  __device__ __forceinline__ void init(double s, double e) {
    amp = s * s;
    cf = (KIND == 1) ? 1.7320508075688772935 / e : (KIND == 4) ? 1.0 / e : (KIND == 5) ? 2.2360679774997896964 / e : -0.5 / (e * e);
  }
  __device__ __forceinline__ void zero() { amp = 0.0; }
  __device__ __forceinline__ double eval(const double* z, const double* x, bool low_d) const {
    double acc = 0.0;
    const int nd = low_d ? 2 : 4;
    for (int k = 0; k < nd; ++k) { const double df = z[k] - x[k]; acc = fma(df, df, acc); }
    if (KIND == 0) return amp * exp(cf * acc);
    const double t = cf * sqrt(acc);
    if (KIND == 1) return amp * (1.0 + t) * exp(-t);
    if (KIND == 4) return amp * exp(-t);
    return amp * (1.0 + t + t * t / 3.0) * exp(-t);
  }
};

struct GramPlan { int tile, step, splits, nt; int64_t cols; };

GramPlan gram_plan(int64_t N, int64_t M, int64_t n_latent, int dtype) {
  GramPlan p;
  p.tile = GR_TILE;
  p.step = dtype == GPZ_F32 ? GramT<float>::BK : GramT<double>::BK;
  p.nt = (int)((M + GR_TILE - 1) / GR_TILE);
  const int64_t tiles = (int64_t)p.nt * (p.nt + 1) / 2 * n_latent;
  int64_t s = (N + GR_SPLIT_COLS - 1) / GR_SPLIT_COLS;
  const int64_t s_occ = (GR_TARGET_WGS + tiles - 1) / tiles;
  if (s_occ > s) s = s_occ;
  int64_t cols = (N + s - 1) / s;
  cols = (cols + p.step - 1) / p.step * p.step;
  if (cols < (int64_t)GR_MIN_STEPS * p.step) cols = (int64_t)GR_MIN_STEPS * p.step;
  p.cols = cols;
  p.splits = (int)((N + cols - 1) / cols);
  return p;
}

inline int gram_rb(int R) { return R <= 16 ? 16 : 64; }

size_t gram_ws_bytes(const GramPlan& p, int64_t n_latent, int R, int dtype) {
  const size_t esz = dtype == GPZ_F32 ? 4 : 8;
  const size_t ntl = (size_t)p.nt * (p.nt + 1) / 2;
  Carver c(nullptr);
  c.take<char>((size_t)p.splits * n_latent * ntl * GR_TILE * GR_TILE * esz);
  c.take<char>((size_t)p.splits * n_latent * p.nt * gram_rb(R) * GR_TILE * esz);
  return c.used();
}

struct GramArgs {
  const void* Z; const void* X; const void* F; const void* sigma; const void* ell;
  void* partG; void* partB;
  double* G; double* b;
  double jitter;
  int64_t M, N, cols;
  int d, R, RB, nt, ntl, Lk, splits;
};

template <typename T, int NBT> struct GramLds {
  static constexpr int BK = GramT<T>::BK, VEC = GramT<T>::VEC;
  static constexpr int LDP = BK + VEC;                    // row pitch: 144 bytes in both precisions, the 16 rows of a fragment read hit 64 banks once
  static constexpr int P_ELEMS = GR_TILE * LDP, F_ELEMS = 16 * NBT * LDP;
  static constexpr int BUF = 2 * P_ELEMS + F_ELEMS;       // panel i, panel j, F chunk
  static constexpr size_t bytes = sizeof(T) * (2 * BUF + 2 * GR_TILE * 4);   // two buffers + the coordinates of both Z blocks
};

template <typename T, int KIND, int NBT>
__global__ __launch_bounds__(GR_THREADS) void gram_kernel(const GramArgs a) {
  using GT = GramT<T>;
  using vec_t = typename GT::vec_t;
  using acc_t = typename GT::acc_t;
  using LD = GramLds<T, NBT>;
  constexpr int VEC = GT::VEC, BK = GT::BK, LDP = LD::LDP, P_ELEMS = LD::P_ELEMS, BUF = LD::BUF;
  constexpr int RB = 16 * NBT;
  constexpr int RG = GR_THREADS / BK;       // rows generated at once (one column per thread)
  constexpr int NM = GR_TILE / RG;          // rows per thread and panel
  constexpr int SLABK = 4 * VEC;            // columns one fragment read covers: lane group q owns VEC consecutive ones
  constexpr int NSLAB = BK / SLABK;
  extern __shared__ __attribute__((aligned(16))) char gram_smem[];
  T* const smem = reinterpret_cast<T*>(gram_smem);
  T* const Zs = smem + 2 * BUF;             // [2][128][4]

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, q = lane >> 4, r16 = lane & 15;
  const int wr = w >> 2, wc = w & 3;
  const int tile = blockIdx.x, split = blockIdx.y, l = blockIdx.z;
  int ti = 0;
  while ((ti + 1) * (ti + 2) / 2 <= tile) ++ti;
  const int tj = tile - ti * (ti + 1) / 2;
  const bool diag = ti == tj;
  const int np = diag ? 1 : 2;
  const int64_t n_begin = (int64_t)split * a.cols;
  const int64_t n_end = (n_begin + a.cols < a.N) ? n_begin + a.cols : a.N;
  const int d = a.d;
  const bool low_d = d <= 2;
  const T* const Xp = static_cast<const T*>(a.X);
  const T* const Fp = static_cast<const T*>(a.F) + (int64_t)l * a.R * a.N;

  GramCov<T, KIND> cov;
  cov.init(static_cast<const T*>(a.sigma)[l], static_cast<const T*>(a.ell)[l]);

  if (tid < 2 * GR_TILE) {
    const int p = tid >> 7, r = tid & 127;
    const int64_t row = (int64_t)(p ? tj : ti) * GR_TILE + r;
    const T* const Zp = static_cast<const T*>(a.Z);
#pragma unroll
    for (int c = 0; c < 4; ++c) Zs[(p * GR_TILE + r) * 4 + c] = (row < a.M && c < d) ? Zp[row * d + c] : (T)0;
  }
  __syncthreads();

  // panels (and, on a diagonal tile, the F chunk) of the BK columns from n0 on
  auto gen = [&](T* buf, int64_t n0) __attribute__((always_inline)) {
    const int k = tid % BK, rg = tid / BK;
    const int64_t n = n0 + k;
    const bool ok = n < n_end;
    T x[4] = {(T)0, (T)0, (T)0, (T)0};
    if (ok) {
#pragma unroll
      for (int c = 0; c < 4; ++c) if (c < d) x[c] = Xp[n * d + c];
    }
    GramCov<T, KIND> cc = cov;
    if (!ok) cc.zero();
    for (int p = 0; p < np; ++p) {
#pragma unroll
      for (int m = 0; m < NM; ++m) {
        const int row = rg + RG * m;
        const T* zp = Zs + (p * GR_TILE + row) * 4;
        const T z[4] = {zp[0], zp[1], zp[2], zp[3]};
        buf[p * P_ELEMS + row * LDP + k] = cc.eval(z, x, low_d);
      }
    }
    if (diag) {
      T* const Fs = buf + 2 * P_ELEMS;
#pragma unroll
      for (int e = tid; e < RB * BK; e += GR_THREADS) {
        const int r = e / BK, kk = e % BK;
        const int64_t nn = n0 + kk;
        Fs[r * LDP + kk] = (r < a.R && nn < n_end) ? Fp[(int64_t)r * a.N + nn] : (T)0;
      }
    }
  };

  acc_t acc[4][2];
  acc_t accb[NBT];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = acc_t{0, 0, 0, 0};
#pragma unroll
  for (int nb = 0; nb < NBT; ++nb) accb[nb] = acc_t{0, 0, 0, 0};

  auto mma = [&](const T* buf) __attribute__((always_inline)) {
    const T* const Pi = buf;
    const T* const Pj = diag ? buf : buf + P_ELEMS;
    const T* const Fs = buf + 2 * P_ELEMS;
#pragma unroll
    for (int s = 0; s < NSLAB; ++s) {
      const int ko = s * SLABK + VEC * q;
      vec_t fa[4], fb[2];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) fa[mi] = *reinterpret_cast<const vec_t*>(Pi + (64 * wr + 16 * mi + r16) * LDP + ko);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) fb[ni] = *reinterpret_cast<const vec_t*>(Pj + (32 * wc + 16 * ni + r16) * LDP + ko);
#pragma unroll
      for (int jj = 0; jj < VEC; ++jj)
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = GT::mma(fa[mi][jj], fb[ni][jj], acc[mi][ni]);
      if (diag) {      // rows 16 w .. 16 w + 15 of b from the same panel
        const vec_t ga = *reinterpret_cast<const vec_t*>(Pi + (16 * w + r16) * LDP + ko);
#pragma unroll
        for (int nb = 0; nb < NBT; ++nb) {
          const vec_t gb = *reinterpret_cast<const vec_t*>(Fs + (16 * nb + r16) * LDP + ko);
#pragma unroll
          for (int jj = 0; jj < VEC; ++jj) accb[nb] = GT::mma(ga[jj], gb[jj], accb[nb]);
        }
      }
    }
  };

  const int nsteps = (int)((n_end - n_begin + BK - 1) / BK);
  gen(smem, n_begin);
  __syncthreads();
  for (int t = 0; t < nsteps; ++t) {
    if (t + 1 < nsteps) gen(smem + ((t + 1) & 1) * BUF, n_begin + (int64_t)(t + 1) * BK);
    mma(smem + (t & 1) * BUF);
    __syncthreads();
  }

  // the split's partial tile: whole 128 x 128 (and RB x 128) images in the workspace, no edge to guard
  T* const pg = static_cast<T*>(a.partG) + (((int64_t)split * a.Lk + l) * a.ntl + tile) * (GR_TILE * GR_TILE);
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        pg[(64 * wr + 16 * mi + GT::crow(q, g)) * GR_TILE + 32 * wc + 16 * ni + r16] = acc[mi][ni][g];
  if (diag) {
    T* const pb = static_cast<T*>(a.partB) + (((int64_t)split * a.Lk + l) * a.nt + ti) * (RB * GR_TILE);
#pragma unroll
    for (int nb = 0; nb < NBT; ++nb)
#pragma unroll
      for (int g = 0; g < 4; ++g) pb[(16 * nb + r16) * GR_TILE + 16 * w + GT::crow(q, g)] = accb[nb][g];
  }
}

template <typename T>
__global__ __launch_bounds__(256) void gram_reduce_kernel(const GramArgs a) {
  const int64_t M = a.M;
  const int64_t nG = (int64_t)a.Lk * M * M, nB = (int64_t)a.Lk * a.R * M;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const T* const pG = static_cast<const T*>(a.partG);
  const T* const pB = static_cast<const T*>(a.partB);
  const int64_t g_split = (int64_t)a.Lk * a.ntl * (GR_TILE * GR_TILE), b_split = (int64_t)a.Lk * a.nt * a.RB * GR_TILE;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nG + nB; e += stride) {
    if (e < nG) {
      const int64_t l = e / (M * M), ij = e - l * M * M;
      const int64_t i = ij / M, j = ij - i * M;
      const int64_t hi = i > j ? i : j, lo = i > j ? j : i;        // the lower-triangle element both (i, j) and (j, i) read
      const int64_t ti = hi / GR_TILE, tj = lo / GR_TILE;
      const int64_t off = (l * a.ntl + ti * (ti + 1) / 2 + tj) * (GR_TILE * GR_TILE) + (hi % GR_TILE) * GR_TILE + lo % GR_TILE;
      double sum = 0.0;
      for (int s = 0; s < a.splits; ++s) sum += (double)pG[s * g_split + off];
      if (i == j) sum += a.jitter;
      a.G[e] = sum;
    } else {
      const int64_t eb = e - nG;
      const int64_t l = eb / (a.R * M), ri = eb - l * a.R * M;
      const int64_t r = ri / M, i = ri - r * M;
      const int64_t off = ((l * a.nt + i / GR_TILE) * a.RB + r) * GR_TILE + i % GR_TILE;
      double sum = 0.0;
      for (int s = 0; s < a.splits; ++s) sum += (double)pB[s * b_split + off];
      a.b[eb] = sum;
    }
  }
}

template <typename T, int KIND, int NBT>
int gram_launch_one(const GramArgs& a, hipStream_t s) {
  static std::mutex mu;
  static bool attr_set[64];
  constexpr size_t lds = GramLds<T, NBT>::bytes;
  int dev = 0;
  GPZ_HIP_OK(hipGetDevice(&dev));
  {
    std::lock_guard<std::mutex> lock(mu);
    if (!attr_set[dev & 63]) {
      GPZ_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(&gram_kernel<T, KIND, NBT>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      attr_set[dev & 63] = true;
    }
  }
  dim3 grid((unsigned)a.ntl, (unsigned)a.splits, (unsigned)a.Lk);
  hipLaunchKernelGGL((gram_kernel<T, KIND, NBT>), grid, dim3(GR_THREADS), lds, s, a);
  GPZ_LAUNCH_OK();
  const int64_t total = (int64_t)a.Lk * a.M * (a.M + a.R);
  int64_t blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL((gram_reduce_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, s, a);
  GPZ_LAUNCH_OK();
  return 0;
}

template <typename T, int KIND>
int gram_launch_kind(const GramArgs& a, hipStream_t s) {
  return a.RB == 16 ? gram_launch_one<T, KIND, 1>(a, s) : gram_launch_one<T, KIND, 4>(a, s);
}

template <typename T>
int gram_launch(int kind, const GramArgs& a, hipStream_t s) {
  switch (kind) {
    case GPZ_KERNEL_RBF: return gram_launch_kind<T, 0>(a, s);
    case GPZ_KERNEL_MATERN32: return gram_launch_kind<T, 1>(a, s);
    case GPZ_KERNEL_MATERN12: return gram_launch_kind<T, 4>(a, s);
    default: return gram_launch_kind<T, 5>(a, s);
  }
}

// argument checks shared by the three entries; 0 when the shape is served
int gram_check_shape(const char* who, int64_t N, int64_t M, int64_t n_latent, int64_t R, int dtype) {
  GPZ_REQUIRE(dtype == GPZ_F32 || dtype == GPZ_F64, "%s: bad dtype %d", who, dtype);
  GPZ_REQUIRE(N >= 1 && N < ((int64_t)1 << 31), "%s: N=%lld unsupported (1 <= N < 2^31)", who, (long long)N);
  GPZ_REQUIRE(M >= 1 && M <= GR_MAX_M, "%s: M=%lld unsupported (1..%lld)", who, (long long)M, (long long)GR_MAX_M);
  GPZ_REQUIRE(n_latent >= 1 && n_latent <= 65535, "%s: n_latent=%lld unsupported (1..65535)", who, (long long)n_latent);
  GPZ_REQUIRE(R >= 1 && R <= GR_MAX_R, "%s: R=%lld right-hand sides per latent unsupported (1..%d)", who, (long long)R, GR_MAX_R);
  return 0;
}

}  // namespace
}  // namespace gpz

extern "C" int gpz_kernel_gram_plan(int64_t N, int64_t M, int32_t n_latent, int32_t dtype, int32_t* tile, int32_t* col_step,
                                    int32_t* n_splits, int64_t* cols_per_split) {
  if (int rc = gpz::gram_check_shape("gpz_kernel_gram_plan", N, M, n_latent, 1, dtype)) return rc;
  const gpz::GramPlan p = gpz::gram_plan(N, M, n_latent, dtype);
  if (tile) *tile = p.tile;
  if (col_step) *col_step = p.step;
  if (n_splits) *n_splits = p.splits;
  if (cols_per_split) *cols_per_split = p.cols;
  return 0;
}

extern "C" size_t gpz_kernel_gram_workspace_bytes(int64_t N, int64_t M, int32_t n_latent, int32_t R, int32_t dtype) {
  if (gpz::gram_check_shape("gpz_kernel_gram_workspace_bytes", N, M, n_latent, R, dtype)) return 0;
  return gpz::gram_ws_bytes(gpz::gram_plan(N, M, n_latent, dtype), n_latent, R, dtype);
}

extern "C" int gpz_kernel_gram(const gpz_kernel_desc* k, const void* Z, int64_t M, const void* X, int64_t N, int32_t d,
                               const void* F, int32_t R, double jitter, double* G, double* b, void* ws, size_t ws_bytes,
                               void* stream) {
  using namespace gpz;
  GPZ_REQUIRE(k, "gpz_kernel_gram: null kernel descriptor");
  GPZ_REQUIRE(k->kind == GPZ_KERNEL_RBF || k->kind == GPZ_KERNEL_MATERN32 || k->kind == GPZ_KERNEL_MATERN12 ||
              k->kind == GPZ_KERNEL_MATERN52,
              "gpz_kernel_gram: kernel kind %d unsupported (stationary kinds 0, 1, 4, 5)", k->kind);
  GPZ_REQUIRE(d >= 1 && d <= 4, "gpz_kernel_gram: input dimension %d unsupported (1..4)", d);
  if (int rc = gram_check_shape("gpz_kernel_gram", N, M, k->n_latent, R, k->dtype)) return rc;
  GPZ_REQUIRE(jitter >= 0.0, "gpz_kernel_gram: jitter must be >= 0");
  GPZ_REQUIRE(Z && X && F && G && b && k->sigma && k->lengthscale, "gpz_kernel_gram: null pointer");
  const GramPlan p = gram_plan(N, M, k->n_latent, k->dtype);
  const size_t need = gram_ws_bytes(p, k->n_latent, R, k->dtype);
  GPZ_REQUIRE(ws && ws_bytes >= need, "gpz_kernel_gram: workspace of %zu bytes, %zu needed", ws_bytes, need);
  const size_t esz = k->dtype == GPZ_F32 ? 4 : 8;
  GramArgs a;
  a.Z = Z; a.X = X; a.F = F; a.sigma = k->sigma; a.ell = k->lengthscale;
  a.G = G; a.b = b; a.jitter = jitter;
  a.M = M; a.N = N; a.cols = p.cols;
  a.d = d; a.R = R; a.RB = gram_rb(R); a.nt = p.nt; a.ntl = p.nt * (p.nt + 1) / 2; a.Lk = k->n_latent; a.splits = p.splits;
  Carver c(ws);
  a.partG = c.take<char>((size_t)p.splits * a.Lk * a.ntl * GR_TILE * GR_TILE * esz);
  a.partB = c.take<char>((size_t)p.splits * a.Lk * p.nt * a.RB * GR_TILE * esz);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (k->dtype == GPZ_F32) return gram_launch<float>(k->kind, a, s);
  return gram_launch<double>(k->kind, a, s);
}
