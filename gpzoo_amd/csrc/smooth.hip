// smooth.hip -- the exact K-nearest mean behind gpzoo.utilities.smooth_spatial_factors (reference utilities.py:50-68,
// sklearn's KNeighborsRegressor.predict with uniform weights): for each of M inducing points the mean of the factors F
// over the K spots nearest to it.  Few queries, many candidates, K up to N: neither gpz_knn (K sorted neighbours in
// registers) nor gpz_spatial_knn (self graph, K <= 32) covers it, so the K-th smallest key is SELECTED, nothing is sorted.
//
//   km_stage    X (N,d) and Z (M,d) once as fp64, compact (the cast is exact)
//   km_query    block = one query (256 threads, a grid-stride loop over the queries).
//               select: an MSB-first radix select on the 64-bit pattern of d^2 (non-negative doubles order like unsigned
//               integers; the sign bit is never set).  Digits: the 11 exponent bits, then the mantissa 8 bits at a time
//               (6 passes) and its last 4.  Each pass recomputes d^2 of every spot (3 d - 1 fp64 operations), counts the
//               spots whose decided bits equal the prefix into an LDS histogram of the next digit -- integer counts, exact
//               in any order -- and a block scan picks the bin that holds the K-th key.  It stops as soon as every spot
//               of that bin is selected (a bin of one key, typically after 2-4 passes) or no bit is left (then the bin is
//               the set of exact ties at the K-th distance).
//               gather: one sweep in index order, 256 spots at a time.  A spot below the bin is selected; of the bin's
//               spots the first `rem` in index order are (an index-order prefix count from wave ballots): exact ties go
//               to the lower index.  The chunk's selected spots are compacted in index order (-> idx) and their rows of F
//               are added into per-thread fp64 accumulators: thread (column, slot) takes every slots-th entry of each
//               chunk, and at the end the slots of a column are added in slot order.
//
// The partition of the spots over threads and the order of every sum are fixed by (N, K, L) alone and no floating-point
// atomic is used: two calls agree bit for bit.  Distances are sklearn's: fp64, (x_k - z_k)^2 rounded on its own, added
// in coordinate order -- this file is built with fp contraction off (gpzoo_amd/build.py).  A NaN d^2 ranks as +inf.
// Nothing of size M x N exists: beyond the inputs and outputs the memory is the staged coordinates, (N + M) d doubles.
#include "common.h"

#include <math.h>

namespace gpz {
namespace {

constexpr int KM_THREADS = 256;
constexpr int KM_WAVES = KM_THREADS / 64;
constexpr int KM_BINS = 2048;         // the widest digit: 11 exponent bits
constexpr int KM_MAX_GRID = 1 << 16;  // queries beyond this many blocks are taken in a grid-stride loop

struct KmPlan {
  double* P;   // (N, d)
  double* Q;   // (M, d)
  size_t bytes;
};

KmPlan km_plan(int64_t N, int64_t M, int d, void* ws) {
  Carver c(ws);
  KmPlan p;
  p.P = c.take<double>(size_t(N) * d);
  p.Q = c.take<double>(size_t(M) * d);
  p.bytes = c.used();
  return p;
}

template <typename T>
__global__ __launch_bounds__(256) void km_stage(const T* __restrict__ src, int64_t n, double* __restrict__ dst) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = double(src[i]);
}

template <int D>
struct KmPoint {
  double x[D];
};

template <int D>
__device__ __forceinline__ KmPoint<D> km_load(const double* __restrict__ P, int64_t n) {
  KmPoint<D> p;
#pragma unroll
  for (int k = 0; k < D; ++k) p.x[k] = P[n * D + k];
  return p;
}

template <int D>
__device__ __forceinline__ uint64_t km_key(const KmPoint<D>& p, const double* q) {
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const double dx = p.x[k] - q[k];
    s = k == 0 ? dx * dx : s + dx * dx;
  }
  if (s != s) s = INFINITY;
  return uint64_t(__double_as_longlong(s));
}

// One count per matching lane into hist[digit].  Lanes that share the digit of the wave's first matching lane are
// counted with one add (ROUNDS times over): the exponent digit, and a set of identical points, put most of a wave into
// one bin, which would otherwise be 64 serialised adds on one LDS address.
template <int ROUNDS>
__device__ __forceinline__ void km_count(uint32_t* hist, bool match, uint32_t digit, int lane) {
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const uint64_t m = __ballot(match);
    if (m == 0) return;
    const int first = __ffsll((unsigned long long)m) - 1;
    const uint32_t d0 = uint32_t(__shfl(int(digit), first));
    const uint64_t same = __ballot(match && digit == d0);
    if (lane == first) atomicAdd(&hist[d0], uint32_t(__popcll(same)));
    match = match && digit != d0;
  }
  if (match) atomicAdd(&hist[digit], 1u);
}

template <int D, typename TF>
__global__ __launch_bounds__(KM_THREADS) void km_query(const double* __restrict__ P, const double* __restrict__ Q, int64_t N,
                                                       int64_t M, const TF* __restrict__ F, int L, int cw, int64_t K,
                                                       double* __restrict__ U, int64_t* __restrict__ idx) {
  __shared__ uint32_t hist[KM_BINS];
  __shared__ uint32_t wtot[KM_WAVES];
  __shared__ uint32_t pick[3];               // the bin of the K-th key, how many of its spots are selected, its count
  __shared__ uint32_t wcnt[2][KM_WAVES][2];  // gather: per chunk parity and wave, spots below the bin / in it
  __shared__ int32_t list[KM_THREADS];       // gather: the chunk's selected spots in index order
  __shared__ double red[KM_THREADS];

  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int col = t % cw, slot = t / cw, slots = KM_THREADS / cw;
  const int64_t chunks = (N + KM_THREADS - 1) / KM_THREADS;

  for (int64_t m = blockIdx.x; m < M; m += gridDim.x) {
    double q[D];
#pragma unroll
    for (int k = 0; k < D; ++k) q[k] = Q[m * D + k];

    // ---- select: prefix = the decided high bits of the K-th key, `low` bits still open, rem = how many spots of the
    // prefix's class are selected (the K - rem spots below it all are)
    uint64_t prefix = 0;
    int low = 63;
    uint32_t rem = uint32_t(K);
    for (int pass = 0;; ++pass) {
      const int bits = pass == 0 ? 11 : (low >= 8 ? 8 : low);
      const int shift = low - bits, nb = 1 << bits;
      for (int b = t; b < nb; b += KM_THREADS) hist[b] = 0;
      __syncthreads();
      KmPoint<D> ahead = km_load<D>(P, t < N ? t : N - 1);     // the next step's spot is loaded one step ahead
      for (int64_t c = 0; c < chunks; ++c) {
        const int64_t n = c * KM_THREADS + t;
        const bool on = n < N;
        const KmPoint<D> p = ahead;
        ahead = km_load<D>(P, n + KM_THREADS < N ? n + KM_THREADS : N - 1);
        const uint64_t key = km_key<D>(p, q);
        const bool match = on && (key >> low) == prefix;
        const uint32_t digit = uint32_t(key >> shift) & uint32_t(nb - 1);
        if (pass == 0) km_count<3>(hist, match, digit, lane);
        else km_count<1>(hist, match, digit, lane);
      }
      __syncthreads();
      // thread t owns `per` consecutive bins; an exclusive block scan of the threads' sums finds the owner of the K-th
      const int per = nb >= KM_THREADS ? nb / KM_THREADS : 1;
      uint32_t own = 0;
      if (t * per < nb)
        for (int j = 0; j < per; ++j) own += hist[t * per + j];
      uint32_t incl = own;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = uint32_t(__shfl_up(int(incl), o));
        if (lane >= o) incl += v;
      }
      if (lane == 63) wtot[w] = incl;
      __syncthreads();
      uint32_t excl = incl - own;
      for (int v = 0; v < w; ++v) excl += wtot[v];
      if (own > 0 && excl < rem && rem <= excl + own) {       // exactly one thread: the counts are >= 0 and sum to >= rem
        uint32_t run = excl;
        for (int j = 0; j < per; ++j) {
          const uint32_t h = hist[t * per + j];
          if (rem <= run + h) {
            pick[0] = uint32_t(t * per + j);
            pick[1] = rem - run;
            pick[2] = h;
            break;
          }
          run += h;
        }
      }
      __syncthreads();
      prefix = (prefix << bits) | pick[0];
      rem = pick[1];
      low = shift;
      if (pick[2] == rem || low == 0) break;                  // (block-uniform)
    }
    const uint64_t lo = prefix << low, hi = lo | ((uint64_t(1) << low) - 1);

    // ---- gather
    double acc = 0.0;
    uint32_t run_tie = 0;      // spots of the class seen so far
    int64_t run_sel = 0;       // spots selected so far
    KmPoint<D> ahead = km_load<D>(P, t < N ? t : N - 1);
    for (int64_t c = 0; c < chunks && run_sel < K; ++c) {
      const int par = int(c & 1);
      const int64_t n = c * KM_THREADS + t;
      const bool on = n < N;
      const KmPoint<D> p = ahead;
      ahead = km_load<D>(P, n + KM_THREADS < N ? n + KM_THREADS : N - 1);
      const uint64_t key = km_key<D>(p, q);
      const bool below = on && key < lo, tie = on && key >= lo && key <= hi;
      const uint64_t mb = __ballot(below), mt = __ballot(tie);
      if (lane == 0) {
        wcnt[par][w][0] = uint32_t(__popcll(mb));
        wcnt[par][w][1] = uint32_t(__popcll(mt));
      }
      __syncthreads();
      // per wave in index order: its ties start at tie0; min(ties, rem - tie0) of them are selected
      uint32_t tie0 = run_tie, before = 0, mine_tie0 = 0, chunk_sel = 0;
#pragma unroll
      for (int v = 0; v < KM_WAVES; ++v) {
        const uint32_t nbel = wcnt[par][v][0], ntie = wcnt[par][v][1];
        const uint32_t room = rem > tie0 ? rem - tie0 : 0;
        const uint32_t sel = nbel + (ntie < room ? ntie : room);
        if (v == w) {
          before = chunk_sel;
          mine_tie0 = tie0;
        }
        chunk_sel += sel;
        tie0 += ntie;
      }
      run_tie = tie0;
      const uint64_t under = (uint64_t(1) << lane) - 1;
      const uint32_t tie_rank = mine_tie0 + uint32_t(__popcll(mt & under));
      const uint32_t room = rem > mine_tie0 ? rem - mine_tie0 : 0;
      const uint32_t ties_under = uint32_t(__popcll(mt & under));
      const uint32_t pos = before + uint32_t(__popcll(mb & under)) + (ties_under < room ? ties_under : room);
      const bool take = below || (tie && tie_rank < rem);
      if (chunk_sel == 0) continue;                           // (block-uniform; wcnt is double-buffered for this)
      if (take && pos < KM_THREADS && run_sel + pos < K) {
        list[pos] = int32_t(n);
        if (idx) idx[m * K + run_sel + pos] = n;
      }
      __syncthreads();
      int64_t cs = chunk_sel;
      if (cs > K - run_sel) cs = K - run_sel;
      if (col < L)
        for (int e = slot; e < int(cs); e += slots) acc += double(F[int64_t(list[e]) * L + col]);
      run_sel += cs;
    }

    red[t] = acc;
    __syncthreads();
    if (slot == 0 && col < L) {
      for (int r = 1; r < slots; ++r) acc += red[r * cw + col];
      U[m * L + col] = acc / double(K);
    }
    __syncthreads();                                          // red, hist and pick are reused by the next query
  }
}

int km_check_args(const char* who, int64_t N, int64_t M, int32_t d, int64_t K, int64_t L, int32_t dtype, int32_t f_dtype) {
  GPZ_REQUIRE(dtype == GPZ_F32 || dtype == GPZ_F64, "%s: unknown dtype %d of the coordinates", who, dtype);
  GPZ_REQUIRE(f_dtype == GPZ_F32 || f_dtype == GPZ_F64, "%s: unknown dtype %d of F", who, f_dtype);
  GPZ_REQUIRE(d >= 1 && d <= 4, "%s: d=%d unsupported (1..4)", who, d);
  GPZ_REQUIRE(N >= 1 && N < (int64_t(1) << 31), "%s: N=%lld unsupported (1 <= N < 2^31)", who, (long long)N);
  GPZ_REQUIRE(K >= 1 && K <= N, "%s: K=%lld unsupported (1 <= K <= N = %lld)", who, (long long)K, (long long)N);
  GPZ_REQUIRE(M >= 1 && M < (int64_t(1) << 31), "%s: M=%lld unsupported (1 <= M < 2^31)", who, (long long)M);
  GPZ_REQUIRE(L >= 1 && L <= 256, "%s: L=%lld unsupported (1..256)", who, (long long)L);
  return 0;
}

template <int D, typename TF>
int km_launch(const KmPlan& pl, int64_t N, int64_t M, const void* F, int64_t L, int64_t K, double* U, int64_t* idx,
              hipStream_t s) {
  int cw = 1;
  while (cw < L) cw <<= 1;                   // columns per row slot: the power of two >= L (<= 256)
  const dim3 grid(unsigned(M < KM_MAX_GRID ? M : KM_MAX_GRID)), block(KM_THREADS);
  hipLaunchKernelGGL((km_query<D, TF>), grid, block, 0, s, pl.P, pl.Q, N, M, static_cast<const TF*>(F), int(L), cw, K, U, idx);
  GPZ_LAUNCH_OK();
  return 0;
}

template <int D>
int km_launch_d(const KmPlan& pl, int64_t N, int64_t M, const void* F, int64_t L, int32_t f_dtype, int64_t K, double* U,
                int64_t* idx, hipStream_t s) {
  return f_dtype == GPZ_F32 ? km_launch<D, float>(pl, N, M, F, L, K, U, idx, s)
                            : km_launch<D, double>(pl, N, M, F, L, K, U, idx, s);
}

template <typename T>
int km_stage_launch(const void* src, int64_t n, double* dst, hipStream_t s) {
  hipLaunchKernelGGL((km_stage<T>), dim3(unsigned((n + 255) / 256)), dim3(256), 0, s, static_cast<const T*>(src), n, dst);
  GPZ_LAUNCH_OK();
  return 0;
}

}  // namespace
}  // namespace gpz

using namespace gpz;

extern "C" size_t gpz_knn_mean_workspace_bytes(int64_t N, int64_t M, int32_t d, int64_t K, int64_t L) {
  if (km_check_args("gpz_knn_mean_workspace_bytes", N, M, d, K, L, GPZ_F64, GPZ_F64)) return 0;
  return km_plan(N, M, d, nullptr).bytes;
}

extern "C" int gpz_knn_mean(const void* X, int64_t N, const void* Z, int64_t M, int32_t d, int32_t dtype, const void* F,
                            int64_t L, int32_t f_dtype, int64_t K, double* U, int64_t* idx, void* ws, size_t ws_bytes,
                            void* stream) {
  GPZ_REQUIRE(X && Z && F && U && ws, "gpz_knn_mean: null pointer");
  if (int rc = km_check_args("gpz_knn_mean", N, M, d, K, L, dtype, f_dtype)) return rc;
  const KmPlan pl = km_plan(N, M, d, ws);
  GPZ_REQUIRE(ws_bytes >= pl.bytes, "gpz_knn_mean: workspace of %zu bytes, %zu needed", ws_bytes, pl.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dtype == GPZ_F32) {
    if (int rc = km_stage_launch<float>(X, N * d, pl.P, s)) return rc;
    if (int rc = km_stage_launch<float>(Z, M * d, pl.Q, s)) return rc;
  } else {
    if (int rc = km_stage_launch<double>(X, N * d, pl.P, s)) return rc;
    if (int rc = km_stage_launch<double>(Z, M * d, pl.Q, s)) return rc;
  }
  switch (d) {
    case 1: return km_launch_d<1>(pl, N, M, F, L, f_dtype, K, U, idx, s);
    case 2: return km_launch_d<2>(pl, N, M, F, L, f_dtype, K, U, idx, s);
    case 3: return km_launch_d<3>(pl, N, M, F, L, f_dtype, K, U, idx, s);
    default: return km_launch_d<4>(pl, N, M, F, L, f_dtype, K, U, idx, s);
  }
}
