// spatial.hip -- the self-kNN graph of the spots, over which the spatial statistics after a fit are taken
// (gpzoo.utilities.dims_autocorr, reference utilities.py:131-156, which goes through squidpy's spatial_neighbors +
// spatial_autocorr(mode="moran"); Moran's I itself is spatial_stats.hip's).
//
//   sk_mark / sk_check   a caller-supplied point order is checked on the device: every entry in [0, N) and every
//                        point named once; anything else is replaced by the identity (same graph, slower search)
//   sk_gather            thread = point of the order: the points in that order as fp64 (4 per row, unused dims 0), their
//                        ORIGINAL indices, and per tile of 64 consecutive points an fp64 bounding box
//   sk_super             wave = 64 tiles: the bounding box of 4096 consecutive points
//   sk_knn               wave = one tile of 64 queries.  Each lane keeps its K best (d^2, original index) pairs sorted in
//                        registers.  Its own tile is searched first, then every super-tile / tile whose box can still
//                        hold a better candidate for SOME lane; one that cannot is skipped.  The candidate loop reads
//                        uniform addresses (scalar loads) and costs 3d - 1 fp64 VALU + one compare per pair.
//
// Distances are sklearn's: fp64, (x_k - y_k)^2 rounded on its own, added in coordinate order -- this file is built with
// fp contraction off (gpzoo_amd/build.py) so no fma fuses a square into the sum.  The tile-skip bound uses the same
// rounded operations on the box's nearest face: rounding is monotone, so bound <= d^2 of every point in the box, and a
// tile is skipped only when the bound is STRICTLY above the lane's K-th best (an equal d^2 with a lower index can enter).
#include "common.h"

#include <math.h>

namespace gpz {
namespace {

constexpr int SK_KMAX = 32;
constexpr int SK_TILE = 64;          // points per tile = queries per wave
constexpr int SK_BOX = 8;            // lo[4], hi[4]

struct SkPlan {
  double* P;          // (N, 4) points in search order
  int32_t* orig;      // (N,) original index of each
  double* box;        // (T, 8)
  double* sbox;       // (S, 8)
  int32_t* seen;      // (N,) order check
  int32_t* bad;       // (1,) the order is not a permutation
  size_t bytes;
};

SkPlan sk_plan(int64_t N, void* ws) {
  const int64_t T = (N + SK_TILE - 1) / SK_TILE, S = (T + SK_TILE - 1) / SK_TILE;
  Carver c(ws);
  SkPlan p;
  p.P = c.take<double>(size_t(N) * 4);
  p.orig = c.take<int32_t>(size_t(N));
  p.box = c.take<double>(size_t(T) * SK_BOX);
  p.sbox = c.take<double>(size_t(S) * SK_BOX);
  p.seen = c.take<int32_t>(size_t(N));
  p.bad = c.take<int32_t>(1);
  p.bytes = c.used();
  return p;
}

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmin(v, __shfl_xor(v, m));
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m));
  return v;
}

__global__ __launch_bounds__(256) void sk_mark(const int64_t* __restrict__ order, int64_t N, int32_t* __restrict__ seen,
                                                int32_t* __restrict__ bad) {
  const int64_t p = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (p >= N) return;
  const int64_t o = order[p];
  if (o < 0 || o >= N) *bad = 1;
  else seen[o] = 1;
}

__global__ __launch_bounds__(256) void sk_check(const int32_t* __restrict__ seen, int64_t N, int32_t* __restrict__ bad) {
  const int64_t p = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (p < N && seen[p] == 0) *bad = 1;       // N entries in range that miss a point: some point is named twice
}

// One 64-thread block per tile.  order == NULL or *bad != 0: the identity.
template <typename T>
__global__ __launch_bounds__(64) void sk_gather(const T* __restrict__ X, int64_t N, int d, const int64_t* __restrict__ order,
                                                const int32_t* __restrict__ bad, double* __restrict__ P,
                                                int32_t* __restrict__ orig, double* __restrict__ box) {
  const int64_t p = int64_t(blockIdx.x) * SK_TILE + threadIdx.x;
  const bool on = p < N;
  const bool ident = order == nullptr || *bad != 0;
  int64_t src = on ? (ident ? p : order[p]) : 0;
  double x[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (on && k < d) x[k] = double(X[src * d + k]);
  if (on) {
    double4 v = make_double4(x[0], x[1], x[2], x[3]);
    reinterpret_cast<double4*>(P)[p] = v;
    orig[p] = int32_t(src);
  }
  for (int k = 0; k < 4; ++k) {              // NaN coordinates are left out of the box (fmin / fmax): see sk_knn
    const double lo = wave_min(on ? x[k] : INFINITY), hi = wave_max(on ? x[k] : -INFINITY);
    if (threadIdx.x == 0) {
      box[blockIdx.x * SK_BOX + k] = lo;
      box[blockIdx.x * SK_BOX + 4 + k] = hi;
    }
  }
}

__global__ __launch_bounds__(64) void sk_super(const double* __restrict__ box, int64_t T, double* __restrict__ sbox) {
  const int64_t t = int64_t(blockIdx.x) * SK_TILE + threadIdx.x;
  const bool on = t < T;
  for (int k = 0; k < 4; ++k) {
    const double lo = wave_min(on ? box[t * SK_BOX + k] : INFINITY);
    const double hi = wave_max(on ? box[t * SK_BOX + 4 + k] : -INFINITY);
    if (threadIdx.x == 0) {
      sbox[blockIdx.x * SK_BOX + k] = lo;
      sbox[blockIdx.x * SK_BOX + 4 + k] = hi;
    }
  }
}

// Lower bound of d^2 between a point q and any point of the box b, in the rounded arithmetic of the distance.
template <int D>
__device__ __forceinline__ double box_bound(const double* q, const double* __restrict__ b) {
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const double g = fmax(fmax(b[k] - q[k], q[k] - b[4 + k]), 0.0);
    s = k == 0 ? g * g : s + g * g;
  }
  return s;
}

// The same between two boxes (the wave's queries and a candidate box).
template <int D>
__device__ __forceinline__ double box_box_bound(const double* qlo, const double* qhi, const double* __restrict__ b) {
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const double g = fmax(fmax(b[k] - qhi[k], qlo[k] - b[4 + k]), 0.0);
    s = k == 0 ? g * g : s + g * g;
  }
  return s;
}

template <int D, int KM>
struct SkLane {
  double q[4];
  double Ld[KM];
  int32_t Li[KM];
  double td;        // K-th best so far (the entry bound), +inf until K candidates are in
  int32_t ti;
  int32_t self;
  bool on;

  __device__ __forceinline__ void insert(double s, int32_t oc, int K) {
#pragma unroll
    for (int i = 0; i < KM; ++i) {
      if (i < K) {
        const bool lt = s < Ld[i] || (s == Ld[i] && oc < Li[i]);
        const double a = lt ? s : Ld[i], b = lt ? Ld[i] : s;
        const int32_t ai = lt ? oc : Li[i], bi = lt ? Li[i] : oc;
        Ld[i] = a;
        Li[i] = ai;
        s = b;
        oc = bi;
        if (i == K - 1) {
          td = Ld[i];
          ti = Li[i];
        }
      }
    }
  }

  // Every candidate of tile t (t is wave-uniform), 8 at a time: their coordinates are loaded (scalar loads) before the
  // distances are formed.  A short tile's tail re-reads its last point and ignores it.
  __device__ __forceinline__ void visit(const double* __restrict__ P, const int32_t* __restrict__ orig, int64_t N, int64_t t,
                                        int K) {
    const int64_t c0 = t * SK_TILE;
    const int n = int(N - c0 < SK_TILE ? N - c0 : SK_TILE);
    for (int j0 = 0; j0 < n; j0 += 8) {
      double c[8][D];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int64_t j = c0 + (j0 + u < n ? j0 + u : n - 1);
#pragma unroll
        for (int k = 0; k < D; ++k) c[u][k] = P[j * 4 + k];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) {
          const double dx = c[u][k] - q[k];
          s = k == 0 ? dx * dx : s + dx * dx;
        }
        if (j0 + u < n && !(s > td)) {        // also NaN: a non-finite pair ranks as +inf, behind every finite one
          const int32_t oc = orig[c0 + j0 + u];
          if (s != s) s = INFINITY;
          if (oc != self && (s < td || (s == td && oc < ti))) insert(s, oc, K);
        }
      }
    }
  }

  // Does any lane's bound to box b allow a candidate in?  (NaN bounds: yes.)
  __device__ __forceinline__ bool wanted(const double* __restrict__ b) const {
    return __ballot(on && !(box_bound<D>(q, b) > td)) != 0;
  }
};

template <int D, int KM>
__global__ __launch_bounds__(256) void sk_knn(const double* __restrict__ P, const int32_t* __restrict__ orig,
                                              const double* __restrict__ box, const double* __restrict__ sbox, int64_t N,
                                              int K, int64_t* __restrict__ idx) {
  const int64_t T = (N + SK_TILE - 1) / SK_TILE, S = (T + SK_TILE - 1) / SK_TILE;
  // readfirstlane: the compiler does not know that threadIdx.x >> 6 is wave-uniform (and would keep every address
  // derived from the tile in vector registers)
  const int64_t w = int64_t(blockIdx.x) * (blockDim.x / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (w >= T) return;
  const int lane = threadIdx.x & 63;
  const int64_t p = w * SK_TILE + lane;

  SkLane<D, KM> L;
  L.on = p < N;
  const int64_t pq = L.on ? p : w * SK_TILE;  // idle lanes shadow the tile's first point and write nothing
#pragma unroll
  for (int k = 0; k < 4; ++k) L.q[k] = P[pq * 4 + k];
  L.self = orig[pq];
#pragma unroll
  for (int i = 0; i < KM; ++i) {
    L.Ld[i] = INFINITY;
    L.Li[i] = INT32_MAX;                     // above every original index (N < 2^31)
  }
  L.td = INFINITY;
  L.ti = INT32_MAX;

  double qlo[4], qhi[4];                     // the wave's query box (NaN coordinates left out)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    qlo[k] = wave_min(L.on ? L.q[k] : INFINITY);
    qhi[k] = wave_max(L.on ? L.q[k] : -INFINITY);
  }

  L.visit(P, orig, N, w, K);                 // own tile first: a tight bound for every lane

  // Tiles of super-tile s0 (the own tile excluded): a lane per tile tests the box against the wave's loosest bound,
  // then each surviving tile is tested per lane before it is searched.
  auto scan = [&](int64_t s0) {
    const double tmax = wave_max(L.on ? L.td : -INFINITY);
    const int64_t t = s0 * SK_TILE + lane;
    const bool cand = t < T && t != w && !(box_box_bound<D>(qlo, qhi, box + t * SK_BOX) > tmax);
    uint64_t m = __ballot(cand);
    while (m) {
      const int b = __ffsll((unsigned long long)m) - 1;
      m &= m - 1;
      const int64_t tb = s0 * SK_TILE + b;
      if (L.wanted(box + tb * SK_BOX)) L.visit(P, orig, N, tb, K);
    }
  };

  const int64_t sw = w / SK_TILE;
  scan(sw);
  for (int64_t s0 = 0; s0 < S; s0 += SK_TILE) {
    const double tmax = wave_max(L.on ? L.td : -INFINITY);
    const int64_t s = s0 + lane;
    const bool cand = s < S && s != sw && !(box_box_bound<D>(qlo, qhi, sbox + s * SK_BOX) > tmax);
    uint64_t m = __ballot(cand);
    while (m) {
      const int b = __ffsll((unsigned long long)m) - 1;
      m &= m - 1;
      const int64_t sb = s0 + b;
      if (L.wanted(sbox + sb * SK_BOX)) scan(sb);
    }
  }

  if (L.on) {
    int64_t* row = idx + int64_t(L.self) * K;
#pragma unroll
    for (int i = 0; i < KM; ++i)
      if (i < K) row[i] = L.Li[i];
  }
}

template <int D>
int sk_launch_d(const SkPlan& pl, int64_t N, int K, int64_t* idx, hipStream_t s) {
  const int64_t T = (N + SK_TILE - 1) / SK_TILE;
  const dim3 grid(unsigned((T + 3) / 4)), block(256);
  if (K <= 8)
    hipLaunchKernelGGL((sk_knn<D, 8>), grid, block, 0, s, pl.P, pl.orig, pl.box, pl.sbox, N, K, idx);
  else if (K <= 16)
    hipLaunchKernelGGL((sk_knn<D, 16>), grid, block, 0, s, pl.P, pl.orig, pl.box, pl.sbox, N, K, idx);
  else
    hipLaunchKernelGGL((sk_knn<D, 32>), grid, block, 0, s, pl.P, pl.orig, pl.box, pl.sbox, N, K, idx);
  GPZ_LAUNCH_OK();
  return 0;
}

int sk_check_args(const char* who, int64_t N, int32_t d, int32_t K, int32_t dtype) {
  GPZ_REQUIRE(dtype == GPZ_F32 || dtype == GPZ_F64, "%s: unknown dtype %d", who, dtype);
  GPZ_REQUIRE(d >= 1 && d <= 4, "%s: d=%d unsupported (1..4)", who, d);
  GPZ_REQUIRE(K >= 1 && K <= SK_KMAX, "%s: K=%d unsupported (1..%d)", who, K, SK_KMAX);
  GPZ_REQUIRE(N > K && N < (int64_t(1) << 31), "%s: N=%lld unsupported (K < N < 2^31)", who, (long long)N);
  return 0;
}

}  // namespace

}  // namespace gpz

using namespace gpz;

extern "C" size_t gpz_spatial_knn_workspace_bytes(int64_t N, int32_t d, int32_t K) {
  if (sk_check_args("gpz_spatial_knn_workspace_bytes", N, d, K, GPZ_F64)) return 0;
  return sk_plan(N, nullptr).bytes;
}

extern "C" int gpz_spatial_knn(const void* X, int64_t N, int32_t d, int32_t K, int32_t dtype, const int64_t* order,
                               int64_t* idx, void* ws, size_t ws_bytes, void* stream) {
  GPZ_REQUIRE(X && idx && ws, "gpz_spatial_knn: null pointer");
  if (int rc = sk_check_args("gpz_spatial_knn", N, d, K, dtype)) return rc;
  const SkPlan pl = sk_plan(N, ws);
  GPZ_REQUIRE(ws_bytes >= pl.bytes, "gpz_spatial_knn: workspace of %zu bytes, %zu needed", ws_bytes, pl.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t T = (N + SK_TILE - 1) / SK_TILE, S = (T + SK_TILE - 1) / SK_TILE;
  const dim3 flat(unsigned((N + 255) / 256)), b256(256);
  if (order) {
    GPZ_HIP_OK(hipMemsetAsync(pl.seen, 0, size_t(N) * sizeof(int32_t), s));
    GPZ_HIP_OK(hipMemsetAsync(pl.bad, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(sk_mark, flat, b256, 0, s, order, N, pl.seen, pl.bad);
    GPZ_LAUNCH_OK();
    hipLaunchKernelGGL(sk_check, flat, b256, 0, s, pl.seen, N, pl.bad);
    GPZ_LAUNCH_OK();
  }
  if (dtype == GPZ_F32)
    hipLaunchKernelGGL((sk_gather<float>), dim3(unsigned(T)), dim3(SK_TILE), 0, s, static_cast<const float*>(X), N, d, order,
                       pl.bad, pl.P, pl.orig, pl.box);
  else
    hipLaunchKernelGGL((sk_gather<double>), dim3(unsigned(T)), dim3(SK_TILE), 0, s, static_cast<const double*>(X), N, d,
                       order, pl.bad, pl.P, pl.orig, pl.box);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(sk_super, dim3(unsigned(S)), dim3(SK_TILE), 0, s, pl.box, T, pl.sbox);
  GPZ_LAUNCH_OK();
  switch (d) {
    case 1: return sk_launch_d<1>(pl, N, K, idx, s);
    case 2: return sk_launch_d<2>(pl, N, K, idx, s);
    case 3: return sk_launch_d<3>(pl, N, K, idx, s);
    default: return sk_launch_d<4>(pl, N, K, idx, s);
  }
}
