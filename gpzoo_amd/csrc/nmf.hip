// nmf.hip -- KL-divergence NMF by multiplicative updates (sklearn's solver='mu', beta_loss='kullback-leibler'), fused.
//
//   X (N,D) >= 0 dense row-major  ~  W (N,L) . H (L,D).   One iteration:
//     P = W H, P[P < EPS] = EPS, Q = X / P;  W *= (Q H^T) / rowsum(H)          (rowsum == 0 -> EPS)
//     P = W H (new W), clamp, Q = X / P;     H *= (W^T Q) / colsum(W)[:, None]  (colsum == 0 -> 1);  H[H < eps64] = 0
//
// P and Q are never stored: each pass forms a 16 x 64 piece of P on the matrix cores (v_mfma_f32_16x16x4_f32 /
// v_mfma_f64_16x16x4_f64, one tile geometry for both), divides X by it on the accumulator registers and feeds the
// quotient into the second product without leaving registers.  Register g of lane (r, q) of a 16 x 16 result holds
// element (row crow(q, g), column r); a product that sums over the ROW index takes exactly that as the B operand of
// k-step g (k slot q <-> row crow(q, g)) when its A operand is read with the same permutation.  So the W pass forms
// P^T (rows = columns of X, which it sums over) and the H pass forms P (rows = rows of X).  A piece is four tiles whose
// column (W pass: row) index interleaves as 4 j + c, c = the tile: a lane's four tiles hold four consecutive entries of
// a row of X, one 16-byte load.
//
//   W pass  workgroup = 64 rows (4 waves x 16), streams H through LDS in chunks of 128 columns.  Reads X once.
//   H pass  workgroup = 256 columns (4 waves x 64) of one slab of rows, streams W through LDS in chunks of 64 rows;
//           writes the slab's (L, 256) partial numerator.  N is cut into slabs so that the grid fills the chip when
//           D / 256 is small.  Reads X once.
//   finish  adds the slabs in slab order, applies the update to H.
// Every sum has a fixed order (no atomics): two calls on the same input agree bit for bit.
//
// L is padded with zero rows / columns to 4 KS, KS (k-steps of the P product) one of 1 2 3 4 5 8 12 16, and to whole
// 16-row tiles in the second product; padded entries of W and H are zeros, a padded row or column of X reads as zero
// and its P as EPS, so Q = 0 there and nothing non-finite reaches a sum.
#include <math.h>

#include "common.h"

namespace gpz {
namespace {

constexpr int NMF_THREADS = 256;
constexpr int NMF_ROWS = 64;     // rows of a W-pass workgroup / of a W chunk in the H pass
constexpr int NMF_WC = 128;      // columns of an H chunk in the W pass
constexpr int NMF_HC = 256;      // columns of an H-pass workgroup
constexpr int NMF_LMAX = 64;
#define NMF_EPS 1.1920928955078125e-07     // np.finfo(np.float32).eps, in both precisions
#define NMF_EPS64 2.220446049250313e-16    // np.finfo(np.float64).eps

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

template <typename T>
struct Mm;
template <>
struct Mm<float> {
  using acc_t = f32x4;
  static __device__ __forceinline__ acc_t mma(float a, float b, acc_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int crow(int q, int g) { return 4 * q + g; }
  static __device__ __forceinline__ void load4(const float* p, float (&v)[4]) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
    v[0] = t[0], v[1] = t[1], v[2] = t[2], v[3] = t[3];
  }
};
template <>
struct Mm<double> {
  using acc_t = f64x4;
  static __device__ __forceinline__ acc_t mma(double a, double b, acc_t c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int crow(int q, int g) { return q + 4 * g; }     // the f64 C/D layout
  static __device__ __forceinline__ void load4(const double* p, double (&v)[4]) {
    const f64x2 a = *reinterpret_cast<const f64x2*>(p), b = *reinterpret_cast<const f64x2*>(p + 2);
    v[0] = a[0], v[1] = a[1], v[2] = b[0], v[3] = b[1];
  }
};

// Four consecutive entries of row n of X from column d (d % 4 == 0); zeros outside (row_ok, D).  `vec`: D % 4 == 0
// and X 16-byte aligned, so the four are one aligned load and lie inside the row together.
template <typename T>
__device__ __forceinline__ void load_x4(const T* __restrict__ X, int64_t n, bool row_ok, int64_t d, int64_t D, bool vec,
                                        T (&v)[4]) {
  v[0] = v[1] = v[2] = v[3] = T(0);
  if (!row_ok || d >= D) return;
  const T* p = X + n * D + d;
  if (vec) {
    Mm<T>::load4(p, v);
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (d + c < D) v[c] = p[c];
  }
}

template <typename T>
__device__ __forceinline__ T clamp_eps(T p) {
  return p < T(NMF_EPS) ? T(NMF_EPS) : p;
}

// ---- W pass ---------------------------------------------------------------------------------------------------------
// wpart (blocks, L): the column sums of the block's 64 NEW rows of W, rows added in order.
template <typename T, int KS>
__global__ __launch_bounds__(NMF_THREADS) void nmf_w_pass(const T* __restrict__ X, T* __restrict__ W, const T* __restrict__ H,
                                                          const double* __restrict__ hsum, double* __restrict__ wpart,
                                                          int64_t N, int64_t D, int L, int vec) {
  using M = Mm<T>;
  using acc_t = typename M::acc_t;
  constexpr int LT = (KS + 3) / 4, L16 = LT * 16;
  constexpr int HS = NMF_WC + 4;                       // row stride of the H chunk: rows 4 banks apart (16-byte reads)
  constexpr int WS = L16 + 1;                          // row stride of the W tile of the epilogue
  static_assert(NMF_ROWS * WS <= L16 * HS, "the epilogue's W tile reuses the H chunk");
  __shared__ __attribute__((aligned(32))) T sH[L16 * HS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
  const int64_t n = int64_t(blockIdx.x) * NMF_ROWS + wave * 16 + r;
  const bool n_ok = n < N;
  T wb[KS];                                            // B[k = 4 s + q][column r] = W[n][4 s + q]
#pragma unroll
  for (int s = 0; s < KS; ++s) wb[s] = (n_ok && 4 * s + q < L) ? W[n * L + 4 * s + q] : T(0);
  acc_t out[LT];
#pragma unroll
  for (int lt = 0; lt < LT; ++lt) out[lt] = acc_t{0, 0, 0, 0};

  T xn[4][4];                                          // [g][c] = X[n][dg + 4 crow(q, g) + c], one step ahead
#pragma unroll
  for (int g = 0; g < 4; ++g) load_x4(X, n, n_ok, int64_t(4 * M::crow(q, g)), D, vec != 0, xn[g]);
  for (int64_t dg = 0; dg < D; dg += 64) {
    const int dl = int(dg % NMF_WC);
    if (dl == 0) {
      __syncthreads();                                 // the previous chunk has been read by every wave
      for (int i = tid; i < L16 * NMF_WC; i += NMF_THREADS) {
        const int l = i / NMF_WC, c = i % NMF_WC;
        const int64_t d = dg + c;
        sH[l * HS + c] = (l < L && d < D) ? H[int64_t(l) * D + d] : T(0);
      }
      __syncthreads();
    }
    T xv[4][4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int c = 0; c < 4; ++c) xv[g][c] = xn[g][c];
    if (dg + 64 < D) {
#pragma unroll
      for (int g = 0; g < 4; ++g) load_x4(X, n, n_ok, dg + 64 + 4 * M::crow(q, g), D, vec != 0, xn[g]);
    }
    // P^T: tile c, row m <-> column dg + 4 m + c of X;  A[m = r][k = 4 s + q] = H[4 s + q][dg + 4 r + c]
    acc_t p[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) p[c] = acc_t{0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      T ha[4];
      M::load4(&sH[(4 * s + q) * HS + dl + 4 * r], ha);
#pragma unroll
      for (int c = 0; c < 4; ++c) p[c] = M::mma(ha[c], wb[s], p[c]);
    }
    // Q^T on the registers, then numerator[l][n] += sum_d H[l][d] Q[n][d]: k-step (g, c), k slot q <-> d = dg + 4 crow(q, g) + c
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      T qv[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) qv[c] = xv[g][c] / clamp_eps<T>(p[c][g]);
#pragma unroll
      for (int lt = 0; lt < LT; ++lt) {
        T hb[4];
        M::load4(&sH[(16 * lt + r) * HS + dl + 4 * M::crow(q, g)], hb);
#pragma unroll
        for (int c = 0; c < 4; ++c) out[lt] = M::mma(hb[c], qv[c], out[lt]);
      }
    }
  }
  // out[lt] register g of lane (r, q): numerator[l = 16 lt + crow(q, g)][n]
  __syncthreads();
  T* sW = sH;
#pragma unroll
  for (int lt = 0; lt < LT; ++lt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int l = 16 * lt + M::crow(q, g);
      T w = T(0);
      if (n_ok && l < L) {
        T den = T(hsum[l]);
        if (den == T(0)) den = T(NMF_EPS);
        w = W[n * L + l] * (out[lt][g] / den);
      }
      sW[(wave * 16 + r) * WS + l] = w;
    }
  __syncthreads();
  const int64_t nb = int64_t(blockIdx.x) * NMF_ROWS;
  for (int i = tid; i < NMF_ROWS * L; i += NMF_THREADS) {
    const int row = i / L, l = i % L;
    if (nb + row < N) W[(nb + row) * L + l] = sW[row * WS + l];
  }
  if (tid < L) {
    double s = 0.0;
    for (int row = 0; row < NMF_ROWS; ++row) s += double(sW[row * WS + tid]);      // rows beyond N hold zeros
    wpart[int64_t(blockIdx.x) * L + tid] = s;
  }
}

// ---- H pass ---------------------------------------------------------------------------------------------------------
// UPDATE: part (slabs, L, D) = the slab's W^T Q.  Otherwise (divergence): dpart (slabs, column blocks, 2) = the block's
// sum of X log(X / P) and of X over the entries with X > EPS, in fp64.
template <typename T, int KS, bool UPDATE>
__global__ __launch_bounds__(NMF_THREADS) void nmf_h_pass(const T* __restrict__ X, const T* __restrict__ W, const T* __restrict__ H,
                                                          T* __restrict__ part, double* __restrict__ dpart, int64_t N, int64_t D,
                                                          int L, int64_t slab_rows, int vec) {
  using M = Mm<T>;
  using acc_t = typename M::acc_t;
  constexpr int LT = (KS + 3) / 4, L16 = LT * 16;
  constexpr int WS = L16 + 1;
  __shared__ T sW[NMF_ROWS * WS];
  __shared__ double red[2][NMF_THREADS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
  const int64_t d0 = int64_t(blockIdx.x) * NMF_HC + wave * 64 + 4 * r;     // this lane's four columns: d0 + c
  const int64_t r_lo = int64_t(blockIdx.y) * slab_rows, r_hi = r_lo + slab_rows < N ? r_lo + slab_rows : N;
  T hb[KS][4];                                         // B[k = 4 s + q][column r of tile c] = H[4 s + q][d0 + c]
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int c = 0; c < 4; ++c) hb[s][c] = (4 * s + q < L && d0 + c < D) ? H[int64_t(4 * s + q) * D + d0 + c] : T(0);
  acc_t out[UPDATE ? LT : 1][4];
#pragma unroll
  for (int lt = 0; lt < (UPDATE ? LT : 1); ++lt)
#pragma unroll
    for (int c = 0; c < 4; ++c) out[lt][c] = acc_t{0, 0, 0, 0};
  double dv = 0.0, dx = 0.0;

  T xn[4][4];                                          // [g][c] = X[n0 + crow(q, g)][d0 + c], one step ahead
#pragma unroll
  for (int g = 0; g < 4; ++g) load_x4(X, r_lo + M::crow(q, g), r_lo + M::crow(q, g) < r_hi, d0, D, vec != 0, xn[g]);
  for (int64_t nb = r_lo; nb < r_hi; nb += NMF_ROWS) {
    __syncthreads();
    for (int i = tid; i < NMF_ROWS * L16; i += NMF_THREADS) {
      const int row = i / L16, l = i % L16;
      sW[row * WS + l] = (nb + row < r_hi && l < L) ? W[(nb + row) * L + l] : T(0);
    }
    __syncthreads();
    for (int sub = 0; sub < NMF_ROWS; sub += 16) {
      const int64_t n0 = nb + sub;
      if (n0 >= r_hi) break;
      T xv[4][4];
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int c = 0; c < 4; ++c) xv[g][c] = xn[g][c];
      if (n0 + 16 < r_hi) {
#pragma unroll
        for (int g = 0; g < 4; ++g)
          load_x4(X, n0 + 16 + M::crow(q, g), n0 + 16 + M::crow(q, g) < r_hi, d0, D, vec != 0, xn[g]);
      }
      // P: row m <-> row n0 + m of X;  A[m = r][k = 4 s + q] = W[n0 + r][4 s + q]
      acc_t p[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) p[c] = acc_t{0, 0, 0, 0};
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const T wa = sW[(sub + r) * WS + 4 * s + q];
#pragma unroll
        for (int c = 0; c < 4; ++c) p[c] = M::mma(wa, hb[s][c], p[c]);
      }
      if (UPDATE) {
        // numerator[l][d] += sum_n W[n][l] Q[n][d]: k-step g, k slot q <-> row n0 + crow(q, g)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          T qv[4];
#pragma unroll
          for (int c = 0; c < 4; ++c) qv[c] = xv[g][c] / clamp_eps<T>(p[c][g]);
#pragma unroll
          for (int lt = 0; lt < LT; ++lt) {
            const T wa = sW[(sub + M::crow(q, g)) * WS + 16 * lt + r];
#pragma unroll
            for (int c = 0; c < 4; ++c) out[lt][c] = M::mma(wa, qv[c], out[lt][c]);
          }
        }
      } else {
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const T x = xv[g][c];
            if (x > T(NMF_EPS)) {
              dv += double(x) * log(double(x) / double(clamp_eps<T>(p[c][g])));
              dx += double(x);
            }
          }
      }
    }
  }
  if (UPDATE) {
    // out[lt][c] register g of lane (r, q): numerator[l = 16 lt + crow(q, g)][d0 + c]
#pragma unroll
    for (int lt = 0; lt < LT; ++lt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int l = 16 * lt + M::crow(q, g);
        if (l >= L) continue;
        T* o = part + (int64_t(blockIdx.y) * L + l) * D + d0;
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (d0 + c < D) o[c] = out[lt][c][g];
      }
  } else {
    red[0][tid] = dv;
    red[1][tid] = dx;
    __syncthreads();
    for (int h = NMF_THREADS / 2; h >= 1; h >>= 1) {
      if (tid < h) {
        red[0][tid] += red[0][tid + h];
        red[1][tid] += red[1][tid + h];
      }
      __syncthreads();
    }
    if (tid == 0) {
      double* o = dpart + (int64_t(blockIdx.y) * gridDim.x + blockIdx.x) * 2;
      o[0] = red[0][0];
      o[1] = red[1][0];
    }
  }
}

// ---- small reductions, each in a fixed order ------------------------------------------------------------------------

// Block l: out[l] = sum over i of src[l * row_stride + i * elem_stride], i < count (strided per thread, then a tree).
// rowsum(H): (row_stride, elem_stride) = (D, 1); the sum of a (count, L) table of partials over its rows: (1, L).
template <typename T>
__global__ __launch_bounds__(NMF_THREADS) void nmf_line_sum(const T* __restrict__ src, int64_t count, int64_t row_stride,
                                                            int64_t elem_stride, double* __restrict__ out) {
  __shared__ double red[NMF_THREADS];
  const T* p = src + int64_t(blockIdx.x) * row_stride;
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < count; i += NMF_THREADS) a += double(p[i * elem_stride]);
  red[threadIdx.x] = a;
  __syncthreads();
  for (int h = NMF_THREADS / 2; h >= 1; h >>= 1) {
    if (threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

// wpart (blocks, L) of W as it stands (the divergence does not follow a W pass): rows of a block added in order.
template <typename T>
__global__ __launch_bounds__(64) void nmf_w_colsum(const T* __restrict__ W, int64_t N, int L, double* __restrict__ wpart) {
  const int l = threadIdx.x;
  if (l >= L) return;
  const int64_t nb = int64_t(blockIdx.x) * NMF_ROWS, ne = nb + NMF_ROWS < N ? nb + NMF_ROWS : N;
  double s = 0.0;
  for (int64_t n = nb; n < ne; ++n) s += double(W[n * L + l]);
  wpart[int64_t(blockIdx.x) * L + l] = s;
}

// H[l][d] *= (sum over the slabs, in slab order, of part[slab][l][d]) / colsum(W)[l];  H < eps64 -> 0.
template <typename T>
__global__ __launch_bounds__(NMF_THREADS) void nmf_h_finish(T* __restrict__ H, const T* __restrict__ part, int64_t slabs,
                                                            const double* __restrict__ wsum, int64_t D, int L) {
  const int64_t d = int64_t(blockIdx.x) * NMF_THREADS + threadIdx.x;
  const int l = blockIdx.y;
  if (d >= D) return;
  double s = 0.0;
  for (int64_t k = 0; k < slabs; ++k) s += double(part[(k * L + l) * D + d]);
  T den = T(wsum[l]);
  if (den == T(0)) den = T(1);
  T h = H[int64_t(l) * D + d] * (T(s) / den);
  if (h < T(NMF_EPS64)) h = T(0);
  H[int64_t(l) * D + d] = h;
}

// sqrt(2 max(res, 0)), res = sum X log(X / P) + colsum(W) . rowsum(H) - sum X  (one block).
__global__ __launch_bounds__(NMF_THREADS) void nmf_div_final(const double* __restrict__ dpart, int64_t parts,
                                                             const double* __restrict__ wsum, const double* __restrict__ hsum,
                                                             int L, double* __restrict__ out) {
  __shared__ double red[2][NMF_THREADS];
  double a = 0.0, b = 0.0;
  for (int64_t i = threadIdx.x; i < parts; i += NMF_THREADS) {
    a += dpart[2 * i];
    b += dpart[2 * i + 1];
  }
  red[0][threadIdx.x] = a;
  red[1][threadIdx.x] = b;
  __syncthreads();
  for (int h = NMF_THREADS / 2; h >= 1; h >>= 1) {
    if (threadIdx.x < h) {
      red[0][threadIdx.x] += red[0][threadIdx.x + h];
      red[1][threadIdx.x] += red[1][threadIdx.x + h];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double swh = 0.0;
    for (int l = 0; l < L; ++l) swh += wsum[l] * hsum[l];
    double res = red[0][0] + (swh - red[1][0]);
    if (!(res > 0.0)) res = res != res ? res : 0.0;
    *out = sqrt(2.0 * res);
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------

struct NmfPlan {
  double* hsum;       // (64,) rowsum(H)
  double* wsum;       // (64,) colsum(W)
  double* wpart;      // (wblocks, L)
  double* dpart;      // (slabs, cblocks, 2)
  void* part;         // (slabs, L, D) of the dtype
  int64_t wblocks, cblocks, slabs, slab_rows;
  size_t bytes;
};

NmfPlan nmf_plan(int64_t N, int64_t D, int64_t L, int32_t dtype, void* ws) {
  Carver c(ws);
  NmfPlan p;
  p.wblocks = (N + NMF_ROWS - 1) / NMF_ROWS;
  p.cblocks = (D + NMF_HC - 1) / NMF_HC;
  // about 1024 workgroups (4 per CU) when N allows, slabs of whole 64-row chunks
  int64_t want = (1024 + p.cblocks - 1) / p.cblocks;
  if (want > p.wblocks) want = p.wblocks;
  if (want < 1) want = 1;
  p.slab_rows = ((N + want - 1) / want + NMF_ROWS - 1) / NMF_ROWS * NMF_ROWS;
  p.slabs = (N + p.slab_rows - 1) / p.slab_rows;
  p.hsum = c.take<double>(NMF_LMAX);
  p.wsum = c.take<double>(NMF_LMAX);
  p.wpart = c.take<double>(size_t(p.wblocks) * L);
  p.dpart = c.take<double>(size_t(p.slabs) * p.cblocks * 2);
  p.part = c.take<char>(size_t(p.slabs) * L * D * (dtype == GPZ_F32 ? 4 : 8));
  p.bytes = c.used();
  return p;
}

int nmf_check_args(const char* who, int64_t N, int64_t D, int64_t L, int32_t dtype) {
  GPZ_REQUIRE(dtype == GPZ_F32 || dtype == GPZ_F64, "%s: unknown dtype %d", who, dtype);
  GPZ_REQUIRE(L >= 1 && L <= NMF_LMAX, "%s: L=%lld unsupported (1..%d)", who, (long long)L, NMF_LMAX);
  GPZ_REQUIRE(N >= 1 && D >= 1 && N < (int64_t(1) << 31) && D < (int64_t(1) << 31) && N * D < (int64_t(1) << 40),
              "%s: N=%lld, D=%lld unsupported (1 <= N, D < 2^31, N D < 2^40)", who, (long long)N, (long long)D);
  return 0;
}

struct NmfArgs {
  const void* X;
  void* W;
  void* H;
  int64_t N, D;
  int L, vec;
};

template <typename T, int KS>
int nmf_iterate(const NmfArgs& a, const NmfPlan& pl, int64_t iters, hipStream_t s) {
  const T* X = static_cast<const T*>(a.X);
  T* W = static_cast<T*>(a.W);
  T* H = static_cast<T*>(a.H);
  T* part = static_cast<T*>(pl.part);
  const dim3 block(NMF_THREADS);
  for (int64_t it = 0; it < iters; ++it) {
    hipLaunchKernelGGL((nmf_line_sum<T>), dim3(unsigned(a.L)), block, 0, s, H, a.D, a.D, int64_t(1), pl.hsum);
    GPZ_LAUNCH_OK();
    hipLaunchKernelGGL((nmf_w_pass<T, KS>), dim3(unsigned(pl.wblocks)), block, 0, s, X, W, H, pl.hsum, pl.wpart, a.N, a.D, a.L,
                       a.vec);
    GPZ_LAUNCH_OK();
    hipLaunchKernelGGL((nmf_line_sum<double>), dim3(unsigned(a.L)), block, 0, s, pl.wpart, pl.wblocks, int64_t(1),
                       int64_t(a.L), pl.wsum);
    GPZ_LAUNCH_OK();
    hipLaunchKernelGGL((nmf_h_pass<T, KS, true>), dim3(unsigned(pl.cblocks), unsigned(pl.slabs)), block, 0, s, X, W, H, part,
                       pl.dpart, a.N, a.D, a.L, pl.slab_rows, a.vec);
    GPZ_LAUNCH_OK();
    hipLaunchKernelGGL((nmf_h_finish<T>), dim3(unsigned((a.D + NMF_THREADS - 1) / NMF_THREADS), unsigned(a.L)), block, 0, s, H,
                       part, pl.slabs, pl.wsum, a.D, a.L);
    GPZ_LAUNCH_OK();
  }
  return 0;
}

template <typename T, int KS>
int nmf_divergence(const NmfArgs& a, const NmfPlan& pl, double* out, hipStream_t s) {
  const T* X = static_cast<const T*>(a.X);
  const T* W = static_cast<const T*>(a.W);
  const T* H = static_cast<const T*>(a.H);
  const dim3 block(NMF_THREADS);
  hipLaunchKernelGGL((nmf_line_sum<T>), dim3(unsigned(a.L)), block, 0, s, H, a.D, a.D, int64_t(1), pl.hsum);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL((nmf_w_colsum<T>), dim3(unsigned(pl.wblocks)), dim3(64), 0, s, W, a.N, a.L, pl.wpart);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL((nmf_line_sum<double>), dim3(unsigned(a.L)), block, 0, s, pl.wpart, pl.wblocks, int64_t(1), int64_t(a.L),
                     pl.wsum);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL((nmf_h_pass<T, KS, false>), dim3(unsigned(pl.cblocks), unsigned(pl.slabs)), block, 0, s, X, W, H,
                     static_cast<T*>(nullptr), pl.dpart, a.N, a.D, a.L, pl.slab_rows, a.vec);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(nmf_div_final, dim3(1), block, 0, s, pl.dpart, pl.slabs * pl.cblocks, pl.wsum, pl.hsum, a.L, out);
  GPZ_LAUNCH_OK();
  return 0;
}

// k-steps of the P product: the smallest instantiated count that holds L
#define NMF_DISPATCH(T, CALL)          \
  const int ks = (a.L + 3) / 4;        \
  if (ks <= 1) return CALL(T, 1);      \
  if (ks <= 2) return CALL(T, 2);      \
  if (ks <= 3) return CALL(T, 3);      \
  if (ks <= 4) return CALL(T, 4);      \
  if (ks <= 5) return CALL(T, 5);      \
  if (ks <= 8) return CALL(T, 8);      \
  if (ks <= 12) return CALL(T, 12);    \
  return CALL(T, 16)

template <typename T>
int nmf_iterate_any(const NmfArgs& a, const NmfPlan& pl, int64_t iters, hipStream_t s) {
#define NMF_CALL_IT(T_, KS_) nmf_iterate<T_, KS_>(a, pl, iters, s)
  NMF_DISPATCH(T, NMF_CALL_IT);
#undef NMF_CALL_IT
}

template <typename T>
int nmf_divergence_any(const NmfArgs& a, const NmfPlan& pl, double* out, hipStream_t s) {
#define NMF_CALL_DIV(T_, KS_) nmf_divergence<T_, KS_>(a, pl, out, s)
  NMF_DISPATCH(T, NMF_CALL_DIV);
#undef NMF_CALL_DIV
}

NmfArgs nmf_args(const void* X, const void* W, const void* H, int64_t N, int64_t D, int64_t L) {
  NmfArgs a;
  a.X = X, a.W = const_cast<void*>(W), a.H = const_cast<void*>(H);
  a.N = N, a.D = D, a.L = int(L);
  a.vec = (D % 4 == 0 && reinterpret_cast<uintptr_t>(X) % 16 == 0) ? 1 : 0;
  return a;
}

}  // namespace
}  // namespace gpz

using namespace gpz;

extern "C" size_t gpz_nmf_kl_workspace_bytes(int64_t N, int64_t D, int64_t L, int32_t dtype) {
  if (nmf_check_args("gpz_nmf_kl_workspace_bytes", N, D, L, dtype)) return 0;
  return nmf_plan(N, D, L, dtype, nullptr).bytes;
}

extern "C" int gpz_nmf_kl_update(const void* X, void* W, void* H, int64_t N, int64_t D, int64_t L, int32_t dtype,
                                 int64_t iters, void* ws, size_t ws_bytes, void* stream) {
  GPZ_REQUIRE(X && W && H && ws, "gpz_nmf_kl_update: null pointer");
  if (int rc = nmf_check_args("gpz_nmf_kl_update", N, D, L, dtype)) return rc;
  GPZ_REQUIRE(iters >= 1, "gpz_nmf_kl_update: iters=%lld unsupported (>= 1)", (long long)iters);
  const NmfPlan pl = nmf_plan(N, D, L, dtype, ws);
  GPZ_REQUIRE(ws_bytes >= pl.bytes, "gpz_nmf_kl_update: workspace of %zu bytes, %zu needed", ws_bytes, pl.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const NmfArgs a = nmf_args(X, W, H, N, D, L);
  return dtype == GPZ_F32 ? nmf_iterate_any<float>(a, pl, iters, s) : nmf_iterate_any<double>(a, pl, iters, s);
}

extern "C" int gpz_nmf_kl_divergence(const void* X, const void* W, const void* H, int64_t N, int64_t D, int64_t L,
                                     int32_t dtype, double* out, void* ws, size_t ws_bytes, void* stream) {
  GPZ_REQUIRE(X && W && H && out && ws, "gpz_nmf_kl_divergence: null pointer");
  if (int rc = nmf_check_args("gpz_nmf_kl_divergence", N, D, L, dtype)) return rc;
  const NmfPlan pl = nmf_plan(N, D, L, dtype, ws);
  GPZ_REQUIRE(ws_bytes >= pl.bytes, "gpz_nmf_kl_divergence: workspace of %zu bytes, %zu needed", ws_bytes, pl.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const NmfArgs a = nmf_args(X, W, H, N, D, L);
  return dtype == GPZ_F32 ? nmf_divergence_any<float>(a, pl, out, s) : nmf_divergence_any<double>(a, pl, out, s);
}
