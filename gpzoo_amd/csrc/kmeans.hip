// kmeans.hip -- k-means++ seeding and Lloyd's iterations behind gpzoo.utilities.kmeans_inducing_points: the inducing
// points Z of a sparse GP as the k-means centres of the spots (the notebooks' sklearn KMeans(n_clusters=M).fit(X)).
//
//   kms_stage     X (N,d) once as fp64, compact (the cast is exact)
//   kms_assign    one point per lane, KMS_B_N points per workgroup; the centres stream through LDS in tiles of KMS_T_C (every
//                 lane reads the same LDS word: a broadcast) and each lane keeps a running (d^2, index) minimum, strict <
//                 in ascending centre index: ties go to the lower index.  When the points alone give fewer than
//                 KMS_SPLIT_WGS workgroups, grid.y splits the centre tiles over several workgroups per point tile, each
//                 writes its (d^2, index) pair and kms_combine takes their minimum in split order (again strict <).
//   kms_sums      one wave per cluster walks the labels in ascending point index; lane j adds the members among the points
//                 n = j (mod KMS_S) into its own fp64 accumulator and the lanes are combined by a fixed shuffle tree.
//   kms_finish    one workgroup: the empty clusters in ascending index, the n_empty farthest points by rounds of a block
//                 arg-max over (d^2 descending, index ascending), the relocation, the new centres, the shift, the stop test.
//   kms_seed_*    one k-means++ step = pick (two-level cumulative sum of closest_d2: block totals, then inside the chosen
//                 block; the T candidates), cand (the T candidates' potentials in one pass over X, per-block partials),
//                 choose (the partials summed in block order, arg-min with ties to the lower t), update (closest_d2 and
//                 its block totals from the winner).
//
// Every launch is a complete step: no kernel waits on another workgroup, an iteration's kernels return at once when the
// caller's state record already holds a stop reason.  No floating-point atomic is used and the order of every sum is fixed
// by the shapes alone: two calls agree bit for bit, and 2 k iterations in one call equal k + k in two.  d^2 is the
// project's kNN distance: fp64, (x_k - c_k)^2 rounded on its own, added in coordinate order -- this file is built with fp
// contraction off (gpzoo_amd/build.py).  A NaN d^2 ranks as +inf.
#include "common.h"

#include <math.h>

namespace gpz {
namespace {

constexpr int KMS_T_C = 256;          // centres per LDS tile of the assignment
constexpr int KMS_B_N = 256;          // points per workgroup of the assignment (one per lane) and per block total of the seeding
constexpr int KMS_S = 64;             // member stride of the cluster sums: lane j of a cluster's wave sums the points j (mod S)
constexpr int KMS_SPLIT_WGS = 1024;   // fewer point tiles than this: the centre tiles are split over grid.y up to about this many workgroups
constexpr int KMS_MAX_T = 32;         // trials per seeding step (2 + floor(ln M) <= 23 for M < 2^31)
constexpr int KMS_FIN = 1024;         // threads of kms_finish

constexpr int KMS_WAVES = KMS_B_N / 64;
constexpr int KMS_FIN_WAVES = KMS_FIN / 64;

struct KmsSplit {
  int splits;           // workgroups per point tile
  int tiles_per_split;  // centre tiles each of them takes
};

KmsSplit kms_split(int64_t N, int64_t M) {
  const int64_t tiles = (N + KMS_B_N - 1) / KMS_B_N, ctiles = (M + KMS_T_C - 1) / KMS_T_C;
  int64_t want = tiles >= KMS_SPLIT_WGS ? 1 : (KMS_SPLIT_WGS + tiles - 1) / tiles;
  if (want > ctiles) want = ctiles;
  KmsSplit s;
  s.tiles_per_split = int((ctiles + want - 1) / want);
  s.splits = int((ctiles + s.tiles_per_split - 1) / s.tiles_per_split);
  return s;
}

struct KmsPlan {
  double* P;         // (N, d) the points as fp64
  double* d2;        // (N) d^2 to the own centre / closest_d2 of the seeding
  double* part_d2;   // (splits, N) the split assignment's partial minima
  int32_t* part_ix;  // (splits, N)
  double* sums;      // (M, d)
  int32_t* counts;   // (M)
  int32_t* empty;    // (M) the empty clusters, ascending
  int32_t* far;      // (M) the relocated points, farthest first
  int32_t* flags;    // [0] a label changed in this iteration; [1] the seeding step's winner
  int32_t* cand;     // (KMS_MAX_T) the seeding step's candidates
  double* bt;        // (nb) block totals (closest_d2, or d^2 for the inertia)
  double* bp;        // (nb) their inclusive prefix
  double* cpart;     // (nb, KMS_MAX_T) per-block potentials of the candidates
  int64_t nb;
  KmsSplit split;
  size_t bytes;
};

KmsPlan kms_plan(int64_t N, int64_t M, int d, void* ws) {
  Carver c(ws);
  KmsPlan p;
  p.nb = (N + KMS_B_N - 1) / KMS_B_N;
  p.split = kms_split(N, M);
  const size_t parts = p.split.splits > 1 ? size_t(p.split.splits) * size_t(N) : 0;
  p.P = c.take<double>(size_t(N) * d);
  p.d2 = c.take<double>(size_t(N));
  p.part_d2 = c.take<double>(parts);
  p.part_ix = c.take<int32_t>(parts);
  p.sums = c.take<double>(size_t(M) * d);
  p.counts = c.take<int32_t>(size_t(M));
  p.empty = c.take<int32_t>(size_t(M));
  p.far = c.take<int32_t>(size_t(M));
  p.flags = c.take<int32_t>(64);
  p.cand = c.take<int32_t>(KMS_MAX_T);
  p.bt = c.take<double>(size_t(p.nb));
  p.bp = c.take<double>(size_t(p.nb));
  p.cpart = c.take<double>(size_t(p.nb) * KMS_MAX_T);
  p.bytes = c.used();
  return p;
}

template <typename T>
__global__ __launch_bounds__(256) void kms_stage(const T* __restrict__ src, int64_t n, double* __restrict__ dst) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = double(src[i]);
}

template <int D>
struct KmsPoint {
  double x[D];
};

template <int D>
__device__ __forceinline__ KmsPoint<D> kms_load(const double* __restrict__ P, int64_t n) {
  KmsPoint<D> p;
#pragma unroll
  for (int k = 0; k < D; ++k) p.x[k] = P[n * D + k];
  return p;
}

template <int D>
__device__ __forceinline__ double kms_dist(const KmsPoint<D>& p, const double* q) {
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const double dx = p.x[k] - q[k];
    s = k == 0 ? dx * dx : s + dx * dx;
  }
  if (s != s) s = INFINITY;
  return s;
}

// lane 0 gets the wave's sum, by one fixed tree
__device__ __forceinline__ double kms_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;
}

// inclusive prefix over the lanes of a wave, by one fixed tree
__device__ __forceinline__ double kms_wave_scan(double v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double u = __shfl_up(v, o);
    if (lane >= o) v += u;
  }
  return v;
}

__device__ __forceinline__ void kms_store_label(int64_t n, double best, int32_t bi, int32_t* __restrict__ labels,
                                                double* __restrict__ d2, int32_t* __restrict__ changed) {
  if (labels[n] != bi) {
    labels[n] = bi;
    atomicOr(changed, 1);
  }
  d2[n] = best;
}

template <int D>
__global__ __launch_bounds__(KMS_B_N) void kms_assign(const double* __restrict__ P, int64_t N, const double* __restrict__ C,
                                                      int32_t M, int tiles_per_split, int splits,
                                                      const gpz_kmeans_state* __restrict__ st, int32_t* __restrict__ labels,
                                                      double* __restrict__ d2, double* __restrict__ part_d2,
                                                      int32_t* __restrict__ part_ix, int32_t* __restrict__ changed) {
  if (st && st->stop) return;                                   // (grid-uniform)
  __shared__ double cs[KMS_T_C * D];
  const int t = threadIdx.x;
  const int64_t n = int64_t(blockIdx.x) * KMS_B_N + t;
  const bool on = n < N;
  const KmsPoint<D> p = kms_load<D>(P, on ? n : N - 1);
  const int64_t c_begin = int64_t(blockIdx.y) * tiles_per_split * KMS_T_C;
  int64_t c_end = c_begin + int64_t(tiles_per_split) * KMS_T_C;
  if (c_end > M) c_end = M;
  double best = INFINITY;
  int32_t bi = int32_t(c_begin);
  for (int64_t c0 = c_begin; c0 < c_end; c0 += KMS_T_C) {
    const int cnt = int(c_end - c0 < KMS_T_C ? c_end - c0 : KMS_T_C);
    __syncthreads();
    for (int i = t; i < cnt * D; i += KMS_B_N) cs[i] = C[c0 * D + i];
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < cnt; ++j) {
      const double s = kms_dist<D>(p, &cs[j * D]);
      if (s < best) {
        best = s;
        bi = int32_t(c0 + j);
      }
    }
  }
  if (!on) return;
  if (splits > 1) {
    part_d2[int64_t(blockIdx.y) * N + n] = best;
    part_ix[int64_t(blockIdx.y) * N + n] = bi;
  } else {
    kms_store_label(n, best, bi, labels, d2, changed);
  }
}

__global__ __launch_bounds__(KMS_B_N) void kms_combine(int64_t N, int splits, const gpz_kmeans_state* __restrict__ st,
                                                       const double* __restrict__ part_d2, const int32_t* __restrict__ part_ix,
                                                       int32_t* __restrict__ labels, double* __restrict__ d2,
                                                       int32_t* __restrict__ changed) {
  if (st && st->stop) return;
  const int64_t n = int64_t(blockIdx.x) * KMS_B_N + threadIdx.x;
  if (n >= N) return;
  double best = part_d2[n];
  int32_t bi = part_ix[n];
  for (int s = 1; s < splits; ++s) {                            // ascending centre ranges: strict < keeps the lower index
    const double v = part_d2[int64_t(s) * N + n];
    if (v < best) {
      best = v;
      bi = part_ix[int64_t(s) * N + n];
    }
  }
  kms_store_label(n, best, bi, labels, d2, changed);
}

// d^2 of every point to the centre its given label names (+inf for a label outside [0, M))
template <int D>
__global__ __launch_bounds__(KMS_B_N) void kms_own_d2(const double* __restrict__ P, int64_t N, const double* __restrict__ C,
                                                      int32_t M, const int32_t* __restrict__ labels, double* __restrict__ d2) {
  const int64_t n = int64_t(blockIdx.x) * KMS_B_N + threadIdx.x;
  if (n >= N) return;
  const int32_t l = labels[n];
  if (l < 0 || l >= M) {
    d2[n] = INFINITY;
    return;
  }
  const KmsPoint<D> p = kms_load<D>(P, n);
  const KmsPoint<D> c = kms_load<D>(C, l);
  d2[n] = kms_dist<D>(p, c.x);
}

template <int D>
__global__ __launch_bounds__(KMS_B_N) void kms_sums(const double* __restrict__ P, int64_t N, const int32_t* __restrict__ labels,
                                                    int32_t M, const gpz_kmeans_state* __restrict__ st,
                                                    double* __restrict__ sums, int32_t* __restrict__ counts) {
  if (st->stop) return;
  const int lane = threadIdx.x & 63;
  const int64_t c = int64_t(blockIdx.x) * KMS_WAVES + (threadIdx.x >> 6);
  if (c >= M) return;                                           // (wave-uniform; no barrier below)
  double acc[D];
#pragma unroll
  for (int k = 0; k < D; ++k) acc[k] = 0.0;
  int32_t cnt = 0;
#pragma unroll 4
  for (int64_t n = lane; n < N; n += KMS_S) {
    if (labels[n] == int32_t(c)) {
#pragma unroll
      for (int k = 0; k < D; ++k) acc[k] += P[n * D + k];
      ++cnt;
    }
  }
#pragma unroll
  for (int k = 0; k < D; ++k) acc[k] = kms_wave_sum(acc[k]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < D; ++k) sums[c * D + k] = acc[k];
    counts[c] = cnt;
  }
}

template <int D>
__global__ __launch_bounds__(KMS_FIN) void kms_finish(const double* __restrict__ P, int64_t N, const int32_t* __restrict__ labels,
                                                      int32_t M, double* __restrict__ C, double* __restrict__ sums,
                                                      int32_t* __restrict__ counts, double* __restrict__ d2,
                                                      int32_t* __restrict__ empty, int32_t* __restrict__ far,
                                                      int32_t* __restrict__ changed, double tol_abs,
                                                      gpz_kmeans_state* __restrict__ st) {
  if (st->stop) return;
  __shared__ double rv[KMS_FIN];
  __shared__ int32_t ri[KMS_FIN];
  __shared__ int32_t wcnt[KMS_FIN_WAVES];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;

  // ---- the empty clusters, ascending
  int32_t run = 0;
  for (int64_t c0 = 0; c0 < M; c0 += KMS_FIN) {
    const int64_t c = c0 + t;
    const bool e = c < M && counts[c] == 0;
    const uint64_t m = __ballot(e);
    if (lane == 0) wcnt[w] = int32_t(__popcll(m));
    __syncthreads();
    int32_t before = 0, total = 0;
#pragma unroll
    for (int v = 0; v < KMS_FIN_WAVES; ++v) {
      if (v < w) before += wcnt[v];
      total += wcnt[v];
    }
    if (e) empty[run + before + int32_t(__popcll(m & ((uint64_t(1) << lane) - 1)))] = int32_t(c);
    run += total;
    __syncthreads();
  }
  const int32_t n_empty = run;                                  // (block-uniform)

  // ---- the n_empty points farthest from their own centres: (d^2 descending, index ascending); taken ones are marked -1
  int32_t n_reloc = 0;
  for (int32_t r = 0; r < n_empty; ++r) {
    double bv = -2.0;
    int32_t bn = 0x7fffffff;
    for (int64_t n = t; n < N; n += KMS_FIN) {
      const double v = d2[n];
      if (v > bv) {                                             // ascending n per thread: strict > keeps the lower index
        bv = v;
        bn = int32_t(n);
      }
    }
    rv[t] = bv;
    ri[t] = bn;
    __syncthreads();
    for (int o = KMS_FIN / 2; o > 0; o >>= 1) {
      if (t < o) {
        const double v = rv[t + o];
        const int32_t i = ri[t + o];
        if (v > rv[t] || (v == rv[t] && i < ri[t])) {
          rv[t] = v;
          ri[t] = i;
        }
      }
      __syncthreads();
    }
    if (r == 0 && !(rv[0] > 0.0)) break;                        // every point on its centre: relocating is pointless
    if (t == 0) {
      far[r] = ri[0];
      d2[ri[0]] = -1.0;
    }
    n_reloc = r + 1;
    __syncthreads();
  }
  if (t == 0) {
    for (int32_t r = 0; r < n_reloc; ++r) {                     // in order: a cluster may lose more than one point
      const int64_t n = far[r];
      const int32_t from = labels[n], to = empty[r];
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const double x = P[n * D + k];
        sums[int64_t(from) * D + k] -= x;
        sums[int64_t(to) * D + k] = x;
      }
      counts[from] -= 1;
      counts[to] = 1;
    }
  }
  __syncthreads();

  // ---- the new centres and the shift
  double sh = 0.0;
  for (int64_t c = t; c < M; c += KMS_FIN) {
    const int32_t cnt = counts[c];
    if (cnt > 0) {
      const double alpha = 1.0 / double(cnt);
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const double cn = sums[c * D + k] * alpha, dc = cn - C[c * D + k];
        sh += dc * dc;
        C[c * D + k] = cn;
      }
    }                                                           // a cluster without a member stays where it is
  }
  rv[t] = sh;
  __syncthreads();
  for (int o = KMS_FIN / 2; o > 0; o >>= 1) {
    if (t < o) rv[t] += rv[t + o];
    __syncthreads();
  }
  if (t == 0) {
    st->iterations += 1;
    st->shift = rv[0];
    st->relocated += n_reloc;
    if (*changed == 0) st->stop = 1;
    else if (rv[0] <= tol_abs) st->stop = 2;
    *changed = 0;
  }
}

// ---- inertia: block totals of d^2, then their sum in block order

__global__ __launch_bounds__(KMS_B_N) void kms_block_totals(const double* __restrict__ v, int64_t N, double* __restrict__ bt) {
  __shared__ double ws[KMS_WAVES];
  const int t = threadIdx.x;
  const int64_t n = int64_t(blockIdx.x) * KMS_B_N + t;
  const double s = kms_wave_sum(n < N ? v[n] : 0.0);
  if ((t & 63) == 0) ws[t >> 6] = s;
  __syncthreads();
  if (t == 0) {
    double a = ws[0];
#pragma unroll
    for (int i = 1; i < KMS_WAVES; ++i) a += ws[i];
    bt[blockIdx.x] = a;
  }
}

__global__ __launch_bounds__(KMS_B_N) void kms_total(const double* __restrict__ bt, int64_t nb, double* __restrict__ out) {
  __shared__ double ws[KMS_WAVES];
  const int t = threadIdx.x;
  double a = 0.0;
  for (int64_t b = t; b < nb; b += KMS_B_N) a += bt[b];
  a = kms_wave_sum(a);
  if ((t & 63) == 0) ws[t >> 6] = a;
  __syncthreads();
  if (t == 0) {
    double s = ws[0];
#pragma unroll
    for (int i = 1; i < KMS_WAVES; ++i) s += ws[i];
    out[0] = s;
  }
}

// ---- seeding

__global__ void kms_seed_first(const double* __restrict__ u, int64_t N, int32_t* __restrict__ win) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int64_t i = int64_t(floor(u[0] * double(N)));
  if (!(i >= 0)) i = 0;
  if (i > N - 1) i = N - 1;
  win[0] = int32_t(i);
}

// closest_d2 <- min(closest_d2, d^2 to the winner) (first: = d^2), its block totals, and the winner into idx_out / C_out
template <int D>
__global__ __launch_bounds__(KMS_B_N) void kms_seed_update(const double* __restrict__ P, int64_t N, const int32_t* __restrict__ win,
                                                           int first, double* __restrict__ closest, double* __restrict__ bt,
                                                           int64_t* __restrict__ idx_out, double* __restrict__ C_out, int64_t c) {
  __shared__ double ws[KMS_WAVES];
  const int t = threadIdx.x;
  const int64_t n = int64_t(blockIdx.x) * KMS_B_N + t;
  const bool on = n < N;
  const int64_t wn = win[0];
  const KmsPoint<D> q = kms_load<D>(P, wn);
  const KmsPoint<D> p = kms_load<D>(P, on ? n : N - 1);
  double v = kms_dist<D>(p, q.x);
  if (on) {
    if (!first) {
      const double old = closest[n];
      if (old < v) v = old;
    }
    closest[n] = v;
  } else {
    v = 0.0;
  }
  const double s = kms_wave_sum(v);
  if ((t & 63) == 0) ws[t >> 6] = s;
  __syncthreads();
  if (t == 0) {
    double a = ws[0];
#pragma unroll
    for (int i = 1; i < KMS_WAVES; ++i) a += ws[i];
    bt[blockIdx.x] = a;
    if (blockIdx.x == 0) {
      idx_out[c] = wn;
#pragma unroll
      for (int k = 0; k < D; ++k) C_out[c * D + k] = q.x[k];
    }
  }
}

// One workgroup: bp = inclusive prefix of the block totals (chunks of KMS_B_N blocks, a wave scan and the waves in order,
// the chunks carried in order), pot = bp[nb - 1]; candidate t = the smallest i with cum[i] >= u[t] pot, where cum inside
// block b is bp[b - 1] + the block's own inclusive prefix (the same scan), clipped to N - 1.
__global__ __launch_bounds__(KMS_B_N) void kms_seed_pick(const double* __restrict__ closest, int64_t N, int64_t nb,
                                                         const double* __restrict__ bt, double* __restrict__ bp,
                                                         const double* __restrict__ u, int T, int32_t* __restrict__ cand) {
  __shared__ double wtot[KMS_WAVES];
  __shared__ double carry_s;
  __shared__ unsigned long long first_s;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  double carry = 0.0;
  for (int64_t b0 = 0; b0 < nb; b0 += KMS_B_N) {
    const int64_t b = b0 + t;
    double v = kms_wave_scan(b < nb ? bt[b] : 0.0, lane);
    if (lane == 63) wtot[w] = v;
    __syncthreads();
    double before = carry;
    for (int x = 0; x < w; ++x) before += wtot[x];
    v += before;
    if (b < nb) bp[b] = v;
    if (t == KMS_B_N - 1) carry_s = v;
    __syncthreads();
    carry = carry_s;
  }
  __syncthreads();                                              // (bp is read below by other threads of this workgroup)
  const double pot = bp[nb - 1];
  for (int tr = 0; tr < T; ++tr) {
    const double target = u[tr] * pot;
    if (t == 0) first_s = ~0ull;
    __syncthreads();
    unsigned long long mine = ~0ull;
    for (int64_t b = t; b < nb; b += KMS_B_N)
      if (bp[b] >= target) {
        mine = (unsigned long long)b;
        break;
      }
    if (mine != ~0ull) atomicMin(&first_s, mine);
    __syncthreads();
    const unsigned long long bsel = first_s;
    __syncthreads();
    if (bsel == ~0ull) {                                        // (block-uniform) rounding put the target past the total
      if (t == 0) cand[tr] = int32_t(N - 1);
      continue;
    }
    const int64_t n = int64_t(bsel) * KMS_B_N + t;
    const bool on = n < N;
    double v = kms_wave_scan(on ? closest[n] : 0.0, lane);
    if (lane == 63) wtot[w] = v;
    if (t == 0) first_s = ~0ull;
    __syncthreads();
    double before = bsel > 0 ? bp[bsel - 1] : 0.0;
    for (int x = 0; x < w; ++x) before += wtot[x];
    v += before;
    if (on && v >= target) atomicMin(&first_s, (unsigned long long)n);
    __syncthreads();
    if (t == 0) {
      int64_t pick = int64_t(bsel) * KMS_B_N + KMS_B_N - 1;      // none inside (the two sums of the block differ in the last bit): its last point
      if (first_s != ~0ull) pick = int64_t(first_s);
      if (pick > N - 1) pick = N - 1;
      cand[tr] = int32_t(pick);
    }
    __syncthreads();
  }
}

// per block and candidate: sum over the block's points of min(closest_d2, d^2 to the candidate)
template <int D>
__global__ __launch_bounds__(KMS_B_N) void kms_seed_cand(const double* __restrict__ P, int64_t N, const double* __restrict__ closest,
                                                         const int32_t* __restrict__ cand, int T, double* __restrict__ cpart) {
  __shared__ double q[KMS_MAX_T * D];
  __shared__ double ws[KMS_WAVES][KMS_MAX_T];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  if (t < T * D) q[t] = P[int64_t(cand[t / D]) * D + t % D];
  __syncthreads();
  const int64_t n = int64_t(blockIdx.x) * KMS_B_N + t;
  const bool on = n < N;
  const KmsPoint<D> p = kms_load<D>(P, on ? n : N - 1);
  const double cl = on ? closest[n] : 0.0;
  for (int tr = 0; tr < T; ++tr) {
    double v = kms_dist<D>(p, &q[tr * D]);
    if (cl < v) v = cl;
    if (!on) v = 0.0;
    v = kms_wave_sum(v);
    if (lane == 0) ws[w][tr] = v;
  }
  __syncthreads();
  if (t < T) {
    double a = ws[0][t];
#pragma unroll
    for (int i = 1; i < KMS_WAVES; ++i) a += ws[i][t];
    cpart[int64_t(blockIdx.x) * KMS_MAX_T + t] = a;
  }
}

// One workgroup: each candidate's potential = its block partials in block order (thread i the blocks i mod KMS_B_N, then
// the fixed tree); the winner is the smallest, ties to the lower t.
__global__ __launch_bounds__(KMS_B_N) void kms_seed_choose(const double* __restrict__ cpart, int64_t nb, int T,
                                                           const int32_t* __restrict__ cand, int32_t* __restrict__ win) {
  __shared__ double ws[KMS_WAVES];
  __shared__ double pots[KMS_MAX_T];
  const int t = threadIdx.x;
  for (int tr = 0; tr < T; ++tr) {
    double a = 0.0;
    for (int64_t b = t; b < nb; b += KMS_B_N) a += cpart[b * KMS_MAX_T + tr];
    a = kms_wave_sum(a);
    if ((t & 63) == 0) ws[t >> 6] = a;
    __syncthreads();
    if (t == 0) {
      double s = ws[0];
#pragma unroll
      for (int i = 1; i < KMS_WAVES; ++i) s += ws[i];
      pots[tr] = s;
    }
    __syncthreads();
  }
  if (t == 0) {
    int best = 0;
    for (int tr = 1; tr < T; ++tr)
      if (pots[tr] < pots[best]) best = tr;
    win[0] = cand[best];
  }
}

// ---- host side

int kms_check_args(const char* who, int64_t N, int32_t d, int32_t dtype, int64_t M) {
  GPZ_REQUIRE(dtype == GPZ_F32 || dtype == GPZ_F64, "%s: unknown dtype %d of X", who, dtype);
  GPZ_REQUIRE(d >= 1 && d <= 4, "%s: d=%d unsupported (1..4)", who, d);
  GPZ_REQUIRE(N >= 1 && N < (int64_t(1) << 31), "%s: N=%lld unsupported (1 <= N < 2^31)", who, (long long)N);
  GPZ_REQUIRE(M >= 1 && M <= N, "%s: M=%lld unsupported (1 <= M <= N = %lld)", who, (long long)M, (long long)N);
  return 0;
}

unsigned kms_blocks(int64_t n, int per) { return unsigned((n + per - 1) / per); }

int kms_stage_x(const void* X, int64_t n, int32_t dtype, double* P, hipStream_t s) {
  if (dtype == GPZ_F32)
    hipLaunchKernelGGL((kms_stage<float>), dim3(kms_blocks(n, 256)), dim3(256), 0, s, static_cast<const float*>(X), n, P);
  else
    hipLaunchKernelGGL((kms_stage<double>), dim3(kms_blocks(n, 256)), dim3(256), 0, s, static_cast<const double*>(X), n, P);
  GPZ_LAUNCH_OK();
  return 0;
}

template <int D>
int kms_assign_launch(const KmsPlan& pl, int64_t N, const double* C, int64_t M, const gpz_kmeans_state* st, int32_t* labels,
                      double* d2, hipStream_t s) {
  const dim3 grid(kms_blocks(N, KMS_B_N), unsigned(pl.split.splits)), block(KMS_B_N);
  hipLaunchKernelGGL((kms_assign<D>), grid, block, 0, s, pl.P, N, C, int32_t(M), pl.split.tiles_per_split, pl.split.splits, st,
                     labels, d2, pl.part_d2, pl.part_ix, pl.flags);
  GPZ_LAUNCH_OK();
  if (pl.split.splits > 1) {
    hipLaunchKernelGGL(kms_combine, dim3(grid.x), block, 0, s, N, pl.split.splits, st, pl.part_d2, pl.part_ix, labels, d2,
                       pl.flags);
    GPZ_LAUNCH_OK();
  }
  return 0;
}

template <int D>
int kms_lloyd_run(const KmsPlan& pl, int64_t N, double* C, int64_t M, double tol_abs, int64_t iters, int32_t* labels,
                  gpz_kmeans_state* st, hipStream_t s) {
  for (int64_t it = 0; it < iters; ++it) {
    if (int rc = kms_assign_launch<D>(pl, N, C, M, st, labels, pl.d2, s)) return rc;
    hipLaunchKernelGGL((kms_sums<D>), dim3(kms_blocks(M, KMS_WAVES)), dim3(KMS_B_N), 0, s, pl.P, N, labels, int32_t(M), st,
                       pl.sums, pl.counts);
    GPZ_LAUNCH_OK();
    hipLaunchKernelGGL((kms_finish<D>), dim3(1), dim3(KMS_FIN), 0, s, pl.P, N, labels, int32_t(M), C, pl.sums, pl.counts, pl.d2,
                       pl.empty, pl.far, pl.flags, tol_abs, st);
    GPZ_LAUNCH_OK();
  }
  return 0;
}

template <int D>
int kms_assign_run(const KmsPlan& pl, int64_t N, const double* C, int64_t M, int keep, int32_t* labels, double* d2,
                   double* inertia, hipStream_t s) {
  if (keep) {
    hipLaunchKernelGGL((kms_own_d2<D>), dim3(kms_blocks(N, KMS_B_N)), dim3(KMS_B_N), 0, s, pl.P, N, C, int32_t(M), labels, d2);
    GPZ_LAUNCH_OK();
  } else if (int rc = kms_assign_launch<D>(pl, N, C, M, nullptr, labels, d2, s)) {
    return rc;
  }
  if (inertia) {
    hipLaunchKernelGGL(kms_block_totals, dim3(unsigned(pl.nb)), dim3(KMS_B_N), 0, s, d2, N, pl.bt);
    GPZ_LAUNCH_OK();
    hipLaunchKernelGGL(kms_total, dim3(1), dim3(KMS_B_N), 0, s, pl.bt, pl.nb, inertia);
    GPZ_LAUNCH_OK();
  }
  return 0;
}

template <int D>
int kms_seed_run(const KmsPlan& pl, int64_t N, int64_t M, int T, const double* u, int64_t* idx_out, double* C_out,
                 hipStream_t s) {
  const dim3 grid(unsigned(pl.nb)), block(KMS_B_N);
  int32_t* win = pl.flags + 1;
  hipLaunchKernelGGL(kms_seed_first, dim3(1), dim3(64), 0, s, u, N, win);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL((kms_seed_update<D>), grid, block, 0, s, pl.P, N, win, 1, pl.d2, pl.bt, idx_out, C_out, int64_t(0));
  GPZ_LAUNCH_OK();
  for (int64_t c = 1; c < M; ++c) {
    hipLaunchKernelGGL(kms_seed_pick, dim3(1), block, 0, s, pl.d2, N, pl.nb, pl.bt, pl.bp, u + c * T, T, pl.cand);
    GPZ_LAUNCH_OK();
    hipLaunchKernelGGL((kms_seed_cand<D>), grid, block, 0, s, pl.P, N, pl.d2, pl.cand, T, pl.cpart);
    GPZ_LAUNCH_OK();
    hipLaunchKernelGGL(kms_seed_choose, dim3(1), block, 0, s, pl.cpart, pl.nb, T, pl.cand, win);
    GPZ_LAUNCH_OK();
    hipLaunchKernelGGL((kms_seed_update<D>), grid, block, 0, s, pl.P, N, win, 0, pl.d2, pl.bt, idx_out, C_out, c);
    GPZ_LAUNCH_OK();
  }
  return 0;
}

}  // namespace
}  // namespace gpz

using namespace gpz;

extern "C" size_t gpz_kmeans_seed_workspace_bytes(int64_t N, int32_t d, int64_t M, int32_t T) {
  if (kms_check_args("gpz_kmeans_seed_workspace_bytes", N, d, GPZ_F64, M)) return 0;
  if (T < 1 || T > KMS_MAX_T) {
    set_error("gpz_kmeans_seed_workspace_bytes: T=%d unsupported (1..%d)", T, KMS_MAX_T);
    return 0;
  }
  return kms_plan(N, M, d, nullptr).bytes;
}

extern "C" int gpz_kmeans_seed(const void* X, int64_t N, int32_t d, int32_t dtype, int64_t M, int32_t T, const double* u,
                               int64_t* idx_out, double* C_out, void* ws, size_t ws_bytes, void* stream) {
  GPZ_REQUIRE(X && u && idx_out && C_out && ws, "gpz_kmeans_seed: null pointer");
  if (int rc = kms_check_args("gpz_kmeans_seed", N, d, dtype, M)) return rc;
  GPZ_REQUIRE(T >= 1 && T <= KMS_MAX_T, "gpz_kmeans_seed: T=%d unsupported (1..%d)", T, KMS_MAX_T);
  const KmsPlan pl = kms_plan(N, M, d, ws);
  GPZ_REQUIRE(ws_bytes >= pl.bytes, "gpz_kmeans_seed: workspace of %zu bytes, %zu needed", ws_bytes, pl.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = kms_stage_x(X, N * d, dtype, pl.P, s)) return rc;
  switch (d) {
    case 1: return kms_seed_run<1>(pl, N, M, T, u, idx_out, C_out, s);
    case 2: return kms_seed_run<2>(pl, N, M, T, u, idx_out, C_out, s);
    case 3: return kms_seed_run<3>(pl, N, M, T, u, idx_out, C_out, s);
    default: return kms_seed_run<4>(pl, N, M, T, u, idx_out, C_out, s);
  }
}

extern "C" size_t gpz_kmeans_lloyd_workspace_bytes(int64_t N, int32_t d, int64_t M) {
  if (kms_check_args("gpz_kmeans_lloyd_workspace_bytes", N, d, GPZ_F64, M)) return 0;
  return kms_plan(N, M, d, nullptr).bytes;
}

extern "C" int gpz_kmeans_lloyd(const void* X, int64_t N, int32_t d, int32_t dtype, double* C, int64_t M, double tol_abs,
                                int64_t iters, int32_t* labels, gpz_kmeans_state* state, void* ws, size_t ws_bytes,
                                void* stream) {
  GPZ_REQUIRE(X && C && labels && state && ws, "gpz_kmeans_lloyd: null pointer");
  if (int rc = kms_check_args("gpz_kmeans_lloyd", N, d, dtype, M)) return rc;
  GPZ_REQUIRE(tol_abs >= 0.0, "gpz_kmeans_lloyd: tol_abs=%g unsupported (>= 0)", tol_abs);
  GPZ_REQUIRE(iters >= 1 && iters <= (int64_t(1) << 20), "gpz_kmeans_lloyd: iters=%lld unsupported (1..2^20)", (long long)iters);
  const KmsPlan pl = kms_plan(N, M, d, ws);
  GPZ_REQUIRE(ws_bytes >= pl.bytes, "gpz_kmeans_lloyd: workspace of %zu bytes, %zu needed", ws_bytes, pl.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = kms_stage_x(X, N * d, dtype, pl.P, s)) return rc;
  GPZ_HIP_OK(hipMemsetAsync(pl.flags, 0, 64 * sizeof(int32_t), s));
  switch (d) {
    case 1: return kms_lloyd_run<1>(pl, N, C, M, tol_abs, iters, labels, state, s);
    case 2: return kms_lloyd_run<2>(pl, N, C, M, tol_abs, iters, labels, state, s);
    case 3: return kms_lloyd_run<3>(pl, N, C, M, tol_abs, iters, labels, state, s);
    default: return kms_lloyd_run<4>(pl, N, C, M, tol_abs, iters, labels, state, s);
  }
}

extern "C" size_t gpz_kmeans_assign_workspace_bytes(int64_t N, int32_t d, int64_t M) {
  if (kms_check_args("gpz_kmeans_assign_workspace_bytes", N, d, GPZ_F64, M)) return 0;
  return kms_plan(N, M, d, nullptr).bytes;
}

extern "C" int gpz_kmeans_assign(const void* X, int64_t N, int32_t d, int32_t dtype, const double* C, int64_t M,
                                 int32_t keep_labels, int32_t* labels, double* d2_out, double* inertia_out, void* ws,
                                 size_t ws_bytes, void* stream) {
  GPZ_REQUIRE(X && C && labels && ws, "gpz_kmeans_assign: null pointer");
  if (int rc = kms_check_args("gpz_kmeans_assign", N, d, dtype, M)) return rc;
  GPZ_REQUIRE(keep_labels == 0 || keep_labels == 1, "gpz_kmeans_assign: keep_labels=%d unsupported (0 or 1)", keep_labels);
  const KmsPlan pl = kms_plan(N, M, d, ws);
  GPZ_REQUIRE(ws_bytes >= pl.bytes, "gpz_kmeans_assign: workspace of %zu bytes, %zu needed", ws_bytes, pl.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = kms_stage_x(X, N * d, dtype, pl.P, s)) return rc;
  double* d2 = d2_out ? d2_out : pl.d2;
  switch (d) {
    case 1: return kms_assign_run<1>(pl, N, C, M, keep_labels, labels, d2, inertia_out, s);
    case 2: return kms_assign_run<2>(pl, N, C, M, keep_labels, labels, d2, inertia_out, s);
    case 3: return kms_assign_run<3>(pl, N, C, M, keep_labels, labels, d2, inertia_out, s);
    default: return kms_assign_run<4>(pl, N, C, M, keep_labels, labels, d2, inertia_out, s);
  }
}
