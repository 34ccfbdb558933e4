// sparse_rows.h -- what the kernels over stored entries (poisson_sparse.hip, nb_sparse.hip, deviance.hip, nb_deviance.hip,
// gaussian_sparse.hip, nmf_sparse.hip) share: the wave-wide sum, the load of a gene's row of W, and the gene pass's work list.
#pragma once
#include "common.h"
#include "vec.h"

namespace gpz {

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {     // every lane ends with the same sum, formed in one fixed tree
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
  return v;
}

// w[0 .. LT) = W[d][0 .. Lt), zeros beyond Lt (LT: the kernel instance's padded factor count)
template <int LT>
__device__ __forceinline__ void load_w(const float* W, int64_t d, int Lt, float (&w)[LT]) {
  const float* wr = W + d * Lt;
  if (Lt == LT) {                           // a multiple of 4: rows start 16-byte aligned
#pragma unroll
    for (int l = 0; l < LT; l += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(wr + l);
      w[l] = v[0]; w[l + 1] = v[1]; w[l + 2] = v[2]; w[l + 3] = v[3];
    }
  } else {
#pragma unroll
    for (int l = 0; l < LT; ++l) w[l] = l < Lt ? wr[l] : 0.f;
  }
}

// The gene pass's work list: row d is cut into ceil(len_d / chunk) chunks of consecutive stored entries.  One workgroup of
// 1024 threads: cstart[d] = number of chunks of the rows before d (cstart[D] = their total, at most nchunks),
// chunk_gene[w] = row of chunk w (-1 past the last one).  nchunks is the caller's bound on the total, which holds whenever
// row_ptr describes nnz entries; clamp_starts (gaussian_sparse.hip) also keeps every cstart[d] at or below it when it does
// not.  A thread reads and rewrites the counts of its own rows only, so no barrier separates the scan from the rewrite.
// (static: one copy per translation unit that launches it.)
static __global__ __launch_bounds__(1024) void chunks_kernel(const int64_t* __restrict__ row_ptr, int64_t D, int64_t nchunks,
                                                             int chunk, bool clamp_starts, int32_t* __restrict__ cstart,
                                                             int32_t* __restrict__ chunk_gene) {
  __shared__ int sh[1024];
  const int t = threadIdx.x;
  // chunks per row, with coalesced independent loads, parked in cstart
  for (int64_t d = t; d < D; d += 1024) cstart[d] = (int32_t)((row_ptr[d + 1] - row_ptr[d] + chunk - 1) / chunk);
  __syncthreads();
  const int64_t per = (D + 1023) / 1024;
  const int64_t d_lo = t * per < D ? t * per : D, d_hi = d_lo + per < D ? d_lo + per : D;
  int mine = 0;
  for (int64_t d = d_lo; d < d_hi; ++d) mine += cstart[d];
  sh[t] = mine;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {      // inclusive scan
    const int v = t >= o ? sh[t - o] : 0;
    __syncthreads();
    sh[t] += v;
    __syncthreads();
  }
  int64_t at = sh[t] - mine;
  const int64_t total = sh[1023];
  for (int64_t d = d_lo; d < d_hi; ++d) {
    const int nc = cstart[d];
    cstart[d] = (int32_t)(clamp_starts && at > nchunks ? nchunks : at);
    for (int c = 0; c < nc; ++c)
      if (at + c < nchunks) chunk_gene[at + c] = (int32_t)d;
    at += nc;
  }
  if (t == 0) cstart[D] = (int32_t)(total < nchunks ? total : nchunks);
  for (int64_t w = total + t; w < nchunks; w += 1024) chunk_gene[w] = -1;
}

}  // namespace gpz
