// poisson_sparse.hip -- the Poisson step of poisson.hip for counts stored as their non-zeros: the same log-likelihood
// and the same four gradients as exact sums over the non-zeros plus O(E Lt B + D Lt) dense terms.
//
// With rate[e,d,n] = V[n] sum_l W[d,l] expF[e,l,n] the sum of the rates factorises,
//   sum_{d,n} rate[e,d,n] = sum_n V[n] t[e,n],   t[e,n] = sum_l c[l] expF[e,l,n],   c[l] = sum_d W[d,l],
// and y log(rate) is non-zero only where y is.  For a non-zero k = (d, n) with count y_k, Z[e,k] = sum_l W[d,l] expF[e,l,n]
// and q[e,k] = y_k / Z[e,k]; with s[l] = sum_{e,n} V[n] expF[e,l,n]:
//   loglik[0]    = (1/E) [ sum_{e,k} y_k log(V[n_k] Z[e,k]) - sum_{e,n} V[n] t[e,n] ],   loglik[1] = sum_k lgamma(y_k + 1)
//   dW[d,l]      = (1/E) [ sum_e sum_{k in row d} q[e,k] expF[e,l,n_k] - s[l] ]
//   dexpF[e,l,n] = (1/E) [ sum_{k in column n} q[e,k] W[d_k,l] - V[n] c[l] ]
//   dV[n]        = (sum_{k in column n} y_k) / V[n] - (1/E) sum_e t[e,n]
//   dmean        = sum_e dexpF expF,   dscale = sum_e dexpF expF eps
//
// The counts arrive in two orders (gpzoo_amd.likelihoods.SparseCounts builds them once): by spot (col_ptr, col_gene, col_val)
// and by gene (row_ptr, row_spot, row_perm = position of the same non-zero in the by-spot order).  A batch is a list of
// distinct spots (idx) with its inverse (pos, -1 outside the batch); both orders stay those of the whole data set.
//
// Launches (fp32, fp64 for the scalars and the column sums, no atomics, no workgroup waits on another, every sum in a
// fixed order -> two calls agree bit for bit):
//   sp_prologue_kernel   expF and expF eps transposed to [B][E][LT] (LT = Lt padded to the kernel instance, zeros beyond
//                        Lt): one spot's samples and factors are one contiguous run
//   sp_colsum_kernel     column sums of W (for c) and, after the spot pass, of V sum_e expF (for s): partials per 256 rows,
//                        then sp_colsum_final_kernel adds them in ascending order
//   chunks_kernel     the gene pass's work list: row d is cut into ceil(len_d / 512) chunks of consecutive non-zeros
//   sp_spot_kernel       one wave per batch spot, lanes stride over the column's non-zeros: log-lik, dV, dmean, dscale
//   sp_gene_kernel       one wave per (gene, chunk): the chunk's partial of sum_e sum_k q expF
//   sp_finish_kernel     dW from the chunk partials in chunk order minus s; the two scalars
// The gene pass forms Z and q again from W[d,:] (wave-uniform) and the spot's exp(F) run, which it reads anyway: a stored
// q would be E gathers through row_perm per non-zero and an (E, nnz) scratch the host cannot size for a batch without
// reading the device.  So there is no array of nnz elements in the workspace at all.
#include "common.h"
#include "mmops.h"
#include "sparse_rows.h"

namespace gpz {

constexpr int SPMAXL = 64;       // factors
constexpr int SP_CHUNK = 512;    // non-zeros of one gene row per wave of the gene pass
constexpr int SP_GROUP_FLOATS = 3072;   // LDS floats per wave of the spot pass: exp(F) and exp(F) eps of one sample group
constexpr int SP_GROUP_MAX = 32;
constexpr int SP_ROWS = 256;     // rows per workgroup of sp_colsum_kernel

typedef float sf32x4 __attribute__((ext_vector_type(4)));

struct SparseArgs {
  const float *mean, *scale, *eps, *W, *V;
  const int64_t* col_ptr; const int32_t* col_gene; const float* col_val;
  const int64_t* row_ptr; const int32_t* row_spot; const int32_t* row_perm;
  const int32_t *idx, *pos;
  float *expT, *xeT;             // [B][E][LT]
  double *cpart, *spart;         // [nbW][LT], [nbS][LT]
  float *csum, *ssum;            // [LT]: c[l] and s[l]
  float* sspot;                  // [B][LT]: V[n] sum_e expF[e,l,n]
  double *ll_spot, *lg_spot;     // [B]
  int32_t *cstart, *chunk_gene;  // [D + 1], [nchunks]
  float* part;                   // [nchunks][LT]
  float *dW, *dmean, *dscale, *dV; double* loglik;
  int64_t N, B, D, nnz, nchunks;
  int Lt, LT, E, EG, nbW, nbS, with_lgamma;
};

static int sp_instance(int Lt) {
  const int sizes[] = {4, 8, 12, 16, 20, 24, 32, 40, 48, 64};
  for (int s : sizes) if (Lt <= s) return s;
  return 0;
}

static int sp_group(int LT, int E) {
  int g = SP_GROUP_FLOATS / (2 * LT);
  if (g > SP_GROUP_MAX) g = SP_GROUP_MAX;
  if (g > E) g = E;
  return g < 1 ? 1 : g;
}

__global__ __launch_bounds__(256) void sp_prologue_kernel(SparseArgs a) {
  __shared__ float xt[SPMAXL][65], et[SPMAXL][65];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int e = blockIdx.x % a.E;
  const int64_t j0 = (int64_t)(blockIdx.x / a.E) * 64;
  const int64_t j = j0 + lane;
  for (int l = wave; l < a.LT; l += 4) {
    float x = 0.f, ep = 0.f;
    if (l < a.Lt && j < a.B) {
      const int64_t ln = (int64_t)l * a.B + j;
      ep = a.eps[(int64_t)e * a.Lt * a.B + ln];
      x = __expf(a.mean[ln] + a.scale[ln] * ep);
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

// part[b][l] = sum over rows b * 256 ... of src[row * stride + l] (l < ncols; zero beyond), in fp64 and a fixed order
__global__ __launch_bounds__(256) void sp_colsum_kernel(const float* src, int64_t R, int stride, int ncols, int LT, double* part) {
  __shared__ double sh[4][64];
  const int l = threadIdx.x & 63, r = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * SP_ROWS, r1 = r0 + SP_ROWS < R ? r0 + SP_ROWS : R;
  double v = 0.0;
  if (l < ncols) {
#pragma unroll 8
    for (int64_t row = r0 + r; row < r1; row += 4) v += (double)src[row * stride + l];
  }
  sh[r][l] = v;
  __syncthreads();
  if (r == 0 && l < LT) part[(int64_t)blockIdx.x * LT + l] = (sh[0][l] + sh[1][l]) + (sh[2][l] + sh[3][l]);
}

// out[l] = sum_b part[b][l] in ascending b (one workgroup of 64 threads)
__global__ __launch_bounds__(64) void sp_colsum_final_kernel(const double* part, int nb, int LT, float* out) {
  const int l = threadIdx.x;
  if (l >= LT) return;
  double v = 0.0;
#pragma unroll 8
  for (int b = 0; b < nb; ++b) v += part[(int64_t)b * LT + l];
  out[l] = (float)v;
}

// Spot pass.  4 waves per workgroup, wave = batch spot j (global spot n = idx[j]).  The spot's exp(F) and exp(F) eps runs go
// through LDS in groups of EG samples; each lane takes every 64th non-zero of the column, reads its gene's row of W and forms
//   Z[e] = w . expF[e],  q[e] = y / Z[e],  A[l] = sum_e q[e] expF[e,l],  B[l] = sum_e q[e] expF[e,l] eps[e,l]
// and adds w[l] A[l], w[l] B[l] to its partial dmean / dscale.  A column has at most D entries and the columns of a count
// matrix are of similar length (a spot's depth varies by a small factor, a gene's expression by four orders of magnitude),
// so columns are not split into chunks.
template <int LT>
__global__ __launch_bounds__(256) void sp_spot_kernel(SparseArgs a) {
  extern __shared__ float sp_smem[];
  float* sc = sp_smem;                                   // c[LT]
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* sx = sp_smem + 64 + wave * 2 * a.EG * LT;       // [EG][LT] exp(F)
  float* se = sx + a.EG * LT;                            // [EG][LT] exp(F) eps
  if (threadIdx.x < 64) sc[threadIdx.x] = (int)threadIdx.x < LT ? a.csum[threadIdx.x] : 0.f;
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
  double ll = 0.0, lg = 0.0;
  float ysum = 0.f, sxl = 0.f, sel = 0.f;                // lane l < LT: sum_e expF[e,l], sum_e expF[e,l] eps[e,l]
  for (int e0 = 0; e0 < a.E; e0 += a.EG) {
    const int ne = a.E - e0 < a.EG ? a.E - e0 : a.EG;
    __syncthreads();                                     // the previous group has been read
    const float* gx = a.expT + (j * a.E + e0) * LT;
    const float* ge = a.xeT + (j * a.E + e0) * LT;
    for (int i = lane; i < ne * LT; i += 64) { sx[i] = gx[i]; se[i] = ge[i]; }
    __syncthreads();
    if (lane < LT)
      for (int e = 0; e < ne; ++e) { sxl += sx[e * LT + lane]; sel += se[e * LT + lane]; }
    for (int64_t k = k0 + lane; k < k1; k += 64) {
      const float y = a.col_val[k];
      if (y == 0.f) continue;                            // an explicit zero: 0 log(.) is never formed
      float w[LT], A[LT], Bv[LT];
      load_w<LT>(a.W, a.col_gene[k], a.Lt, w);
#pragma unroll
      for (int l = 0; l < LT; ++l) A[l] = Bv[l] = 0.f;
      float slog = 0.f;
      for (int e = 0; e < ne; ++e) {
        const sf32x4* xp = reinterpret_cast<const sf32x4*>(sx + e * LT);
        const sf32x4* ep = reinterpret_cast<const sf32x4*>(se + e * LT);
        float z = 0.f;
#pragma unroll
        for (int l = 0; l < LT; l += 4) {
          const sf32x4 x = xp[l / 4];
          z = __builtin_fmaf(w[l], x[0], z); z = __builtin_fmaf(w[l + 1], x[1], z);
          z = __builtin_fmaf(w[l + 2], x[2], z); z = __builtin_fmaf(w[l + 3], x[3], z);
        }
        slog += __logf(vn * z);
        const float q = y * __builtin_amdgcn_rcpf(z);
#pragma unroll
        for (int l = 0; l < LT; l += 4) {
          const sf32x4 x = xp[l / 4], xe = ep[l / 4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            A[l + i] = __builtin_fmaf(q, x[i], A[l + i]);
            Bv[l + i] = __builtin_fmaf(q, xe[i], Bv[l + i]);
          }
        }
      }
      ll += (double)(y * slog);
#pragma unroll
      for (int l = 0; l < LT; ++l) {
        dm[l] = __builtin_fmaf(w[l], A[l], dm[l]);
        ds[l] = __builtin_fmaf(w[l], Bv[l], ds[l]);
      }
      if (e0 == 0) {
        ysum += y;
        if (a.with_lgamma) lg += (double)lgammaf(y + 1.f);
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
  const float cl = lane < LT ? sc[lane] : 0.f;
  const float tsum = wave_sum(cl * sxl);              // sum_e t[e,n]
  ysum = wave_sum(ysum);
  ll = wave_sum(ll);
  lg = wave_sum(lg);
  if (!valid) return;
  if (lane < a.Lt) {
    a.dmean[(int64_t)lane * a.B + j] = inv_e * (my_dm - vn * cl * sxl);
    a.dscale[(int64_t)lane * a.B + j] = inv_e * (my_ds - vn * cl * sel);
  }
  if (lane < LT) a.sspot[j * LT + lane] = vn * sxl;
  if (lane == 0) {
    a.dV[j] = ysum / vn - inv_e * tsum;
    a.ll_spot[j] = (ll - (double)vn * (double)tsum) * (double)inv_e;
    a.lg_spot[j] = lg;
  }
}

// Gene pass.  4 waves per workgroup, wave = chunk w of the work list: at most 512 consecutive non-zeros of one gene row.
// The wave first packs the chunk's entries that lie in the batch (pos[n] >= 0) and are not stored zeros into LDS, in their
// order, then every lane takes every 64th packed entry: with a batch of a fifth of the spots four lanes in five would
// otherwise idle through the arithmetic.
template <int LT>
__global__ __launch_bounds__(256) void sp_gene_kernel(SparseArgs a) {
  __shared__ int32_t lj[4][SP_CHUNK];
  __shared__ float ly[4][SP_CHUNK];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t wi = (int64_t)blockIdx.x * 4 + wave;
  const int g = wi < a.nchunks ? a.chunk_gene[wi] : -1;
  int cnt = 0;
  if (g >= 0) {
    const int64_t p0 = a.row_ptr[g] + (wi - a.cstart[g]) * SP_CHUNK;
    const int64_t pe = a.row_ptr[g + 1], p1 = p0 + SP_CHUNK < pe ? p0 + SP_CHUNK : pe;
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
    }
  }
  __syncthreads();                 // every wave, with or without a chunk, arrives here exactly once
  if (g < 0) return;
  float w[LT], acc[LT];
  load_w<LT>(a.W, g, a.Lt, w);
#pragma unroll
  for (int l = 0; l < LT; ++l) acc[l] = 0.f;
  for (int i = lane; i < cnt; i += 64) {
    const int64_t j = lj[wave][i];
    const float y = ly[wave][i];
    const sf32x4* xp = reinterpret_cast<const sf32x4*>(a.expT + j * a.E * LT);
    for (int e = 0; e < a.E; ++e, xp += LT / 4) {
      float x[LT];
      float z = 0.f;
#pragma unroll
      for (int l = 0; l < LT; l += 4) {
        const sf32x4 v = xp[l / 4];
        x[l] = v[0]; x[l + 1] = v[1]; x[l + 2] = v[2]; x[l + 3] = v[3];
        z = __builtin_fmaf(w[l], v[0], z); z = __builtin_fmaf(w[l + 1], v[1], z);
        z = __builtin_fmaf(w[l + 2], v[2], z); z = __builtin_fmaf(w[l + 3], v[3], z);
      }
      const float q = y * __builtin_amdgcn_rcpf(z);
#pragma unroll
      for (int l = 0; l < LT; ++l) acc[l] = __builtin_fmaf(q, x[l], acc[l]);
    }
  }
  float mine = 0.f;
#pragma unroll
  for (int l = 0; l < LT; ++l) {
    const float t = wave_sum(acc[l]);
    if (lane == l) mine = t;
  }
  if (lane < LT) a.part[wi * LT + lane] = mine;
}

// dW[d,l] = (1/E) (sum of the row's chunk partials in chunk order - s[l]); workgroup 0 also adds the spots' scalars
__global__ __launch_bounds__(256) void sp_finish_kernel(SparseArgs a) {
  __shared__ double sh[8];
  __shared__ float ss[64];
  if (threadIdx.x < 64) ss[threadIdx.x] = (int)threadIdx.x < a.LT ? a.ssum[threadIdx.x] : 0.f;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < a.D * a.Lt) {
    const int64_t d = i / a.Lt;
    const int l = (int)(i - d * a.Lt);
    float v = 0.f;
    for (int64_t c = a.cstart[d]; c < a.cstart[d + 1]; ++c) v += a.part[c * a.LT + l];
    a.dW[i] = (v - ss[l]) * (1.f / (float)a.E);
  }
  if (blockIdx.x == 0) {
    double v = 0.0, vg = 0.0;
    for (int64_t j = threadIdx.x; j < a.B; j += 256) { v += a.ll_spot[j]; vg += a.lg_spot[j]; }
    const double t = block_sum(v, sh);
    const double tg = block_sum(vg, sh);
    if (threadIdx.x == 0) { a.loglik[0] = t; a.loglik[1] = tg; }
  }
}

struct SparsePlan { int LT, EG, nbW, nbS; int64_t nchunks; size_t bytes; };

static SparsePlan sparse_plan(int64_t B, int64_t D, int Lt, int E, int64_t nnz, SparseArgs* a, void* ws) {
  SparsePlan p;
  p.LT = sp_instance(Lt);
  p.EG = sp_group(p.LT, E);
  p.nbW = (int)((D + SP_ROWS - 1) / SP_ROWS);
  p.nbS = (int)((B + SP_ROWS - 1) / SP_ROWS);
  p.nchunks = D + nnz / SP_CHUNK;            // sum_d ceil(len_d / C) <= D + floor(nnz / C)
  Carver c(ws);
  float* expT = c.take<float>((size_t)B * E * p.LT);
  float* xeT = c.take<float>((size_t)B * E * p.LT);
  double* cpart = c.take<double>((size_t)p.nbW * p.LT);
  double* spart = c.take<double>((size_t)p.nbS * p.LT);
  float* csum = c.take<float>(SPMAXL);
  float* ssum = c.take<float>(SPMAXL);
  float* sspot = c.take<float>((size_t)B * p.LT);
  double* ll_spot = c.take<double>((size_t)B);
  double* lg_spot = c.take<double>((size_t)B);
  int32_t* cstart = c.take<int32_t>((size_t)D + 1);
  int32_t* chunk_gene = c.take<int32_t>((size_t)p.nchunks);
  float* part = c.take<float>((size_t)p.nchunks * p.LT);
  p.bytes = c.used();
  if (a) {
    a->expT = expT; a->xeT = xeT; a->cpart = cpart; a->spart = spart; a->csum = csum; a->ssum = ssum; a->sspot = sspot; a->ll_spot = ll_spot;
    a->lg_spot = lg_spot; a->cstart = cstart; a->chunk_gene = chunk_gene; a->part = part;
    a->LT = p.LT; a->EG = p.EG; a->nbW = p.nbW; a->nbS = p.nbS; a->nchunks = p.nchunks;
  }
  return p;
}

static int sparse_check_shape(const char* who, int64_t N, int64_t B, int64_t D, int Lt, int E, int64_t nnz) {
  GPZ_REQUIRE(N >= 1 && B >= 1 && D >= 1 && nnz >= 0, "%s: bad extents (N = %lld, B = %lld, D = %lld, nnz = %lld)", who,
              (long long)N, (long long)B, (long long)D, (long long)nnz);
  GPZ_REQUIRE(B <= N, "%s: a batch of %lld distinct spots out of %lld", who, (long long)B, (long long)N);
  GPZ_REQUIRE(Lt >= 1 && Lt <= SPMAXL, "%s: %d factors unsupported (1..%d)", who, Lt, SPMAXL);
  GPZ_REQUIRE(E >= 1, "%s: %d samples", who, E);
  GPZ_REQUIRE(N < (1ll << 31) && D < (1ll << 31) && nnz < (1ll << 31) && D + nnz / SP_CHUNK < (1ll << 31),
              "%s: spots, genes and non-zeros are indexed with 32 bits", who);
  GPZ_REQUIRE((B + 63) / 64 * E < (1ll << 31) && (double)B * E * SPMAXL < 9.0e15, "%s: B * E too large for one call", who);
  return 0;
}

template <int LT>
static int sparse_passes(const SparseArgs& a, hipStream_t s) {
  const size_t lds = sizeof(float) * (64 + (size_t)4 * 2 * a.EG * LT);
  hipLaunchKernelGGL((sp_spot_kernel<LT>), dim3((unsigned)((a.B + 3) / 4)), dim3(256), lds, s, a);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(sp_colsum_kernel, dim3((unsigned)a.nbS), dim3(256), 0, s, a.sspot, a.B, LT, LT, LT, a.spart);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(sp_colsum_final_kernel, dim3(1), dim3(64), 0, s, a.spart, a.nbS, LT, a.ssum);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL((sp_gene_kernel<LT>), dim3((unsigned)((a.nchunks + 3) / 4)), dim3(256), 0, s, a);
  GPZ_LAUNCH_OK();
  return 0;
}

}  // namespace gpz

using namespace gpz;

extern "C" int gpz_poisson_nsf_sparse_plan(int64_t N, int64_t B, int64_t D, int32_t Lt, int32_t E, int64_t nnz,
                                           int32_t* gene_chunk, int32_t* spot_chunk, int64_t* n_gene_chunks,
                                           int32_t* samples_per_group, int32_t* factors_padded) {
  if (int rc = sparse_check_shape("gpz_poisson_nsf_sparse_plan", N, B, D, Lt, E, nnz)) return rc;
  const SparsePlan p = sparse_plan(B, D, Lt, E, nnz, nullptr, nullptr);
  if (gene_chunk) *gene_chunk = SP_CHUNK;
  if (spot_chunk) *spot_chunk = 0;
  if (n_gene_chunks) *n_gene_chunks = p.nchunks;
  if (samples_per_group) *samples_per_group = p.EG;
  if (factors_padded) *factors_padded = p.LT;
  return 0;
}

extern "C" size_t gpz_poisson_nsf_sparse_workspace_bytes(int64_t N, int64_t B, int64_t D, int64_t nnz, int32_t Lt, int32_t E) {
  if (sparse_check_shape("gpz_poisson_nsf_sparse_workspace_bytes", N, B, D, Lt, E, nnz)) return 0;
  return sparse_plan(B, D, Lt, E, nnz, nullptr, nullptr).bytes;
}

extern "C" int gpz_poisson_nsf_sparse(const float* mean, const float* scale, const float* eps, const float* W, const float* V,
                                      const int64_t* col_ptr, const int32_t* col_gene, const float* col_val,
                                      const int64_t* row_ptr, const int32_t* row_spot, const int32_t* row_perm,
                                      const int32_t* idx, const int32_t* pos, int64_t N, int64_t B, int64_t D, int64_t nnz,
                                      int32_t Lt, int32_t E, int32_t with_lgamma, double* loglik, float* dmean, float* dscale,
                                      float* dW, float* dV, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = sparse_check_shape("gpz_poisson_nsf_sparse", N, B, D, Lt, E, nnz)) return rc;
  GPZ_REQUIRE(mean && scale && eps && W && V && col_ptr && row_ptr && loglik && dmean && dscale && dW && dV && ws,
              "gpz_poisson_nsf_sparse: null pointer");
  GPZ_REQUIRE(nnz == 0 || (col_gene && col_val && row_spot && row_perm), "gpz_poisson_nsf_sparse: null pointer (non-zeros)");
  GPZ_REQUIRE((idx == nullptr) == (pos == nullptr), "gpz_poisson_nsf_sparse: idx and pos come together (both null: all spots)");
  GPZ_REQUIRE(idx || B == N, "gpz_poisson_nsf_sparse: B = %lld of N = %lld spots needs idx and pos", (long long)B, (long long)N);
  // rows of W are read 16 bytes at a time when Lt is the instance's size; the workspace is carved into aligned pieces
  GPZ_REQUIRE(((reinterpret_cast<uintptr_t>(W) | reinterpret_cast<uintptr_t>(ws)) & 15) == 0,
              "gpz_poisson_nsf_sparse: W and the workspace must be 16-byte aligned");
  SparseArgs a;
  const SparsePlan p = sparse_plan(B, D, Lt, E, nnz, &a, ws);
  GPZ_REQUIRE(ws_bytes >= p.bytes, "gpz_poisson_nsf_sparse: workspace of %zu bytes, %zu needed", ws_bytes, p.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  a.mean = mean; a.scale = scale; a.eps = eps; a.W = W; a.V = V;
  a.col_ptr = col_ptr; a.col_gene = col_gene; a.col_val = col_val;
  a.row_ptr = row_ptr; a.row_spot = row_spot; a.row_perm = row_perm; a.idx = idx; a.pos = pos;
  a.dW = dW; a.dmean = dmean; a.dscale = dscale; a.dV = dV; a.loglik = loglik;
  a.N = N; a.B = B; a.D = D; a.nnz = nnz; a.Lt = Lt; a.E = E; a.with_lgamma = with_lgamma;
  hipLaunchKernelGGL(sp_prologue_kernel, dim3((unsigned)((B + 63) / 64 * E)), dim3(256), 0, s, a);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(sp_colsum_kernel, dim3((unsigned)a.nbW), dim3(256), 0, s, W, D, (int)Lt, (int)Lt, a.LT, a.cpart);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(sp_colsum_final_kernel, dim3(1), dim3(64), 0, s, a.cpart, a.nbW, a.LT, a.csum);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(chunks_kernel, dim3(1), dim3(1024), 0, s, a.row_ptr, a.D, a.nchunks, SP_CHUNK, false, a.cstart, a.chunk_gene);
  GPZ_LAUNCH_OK();
  int rc;
  switch (a.LT) {
    case 4: rc = sparse_passes<4>(a, s); break;
    case 8: rc = sparse_passes<8>(a, s); break;
    case 12: rc = sparse_passes<12>(a, s); break;
    case 16: rc = sparse_passes<16>(a, s); break;
    case 20: rc = sparse_passes<20>(a, s); break;
    case 24: rc = sparse_passes<24>(a, s); break;
    case 32: rc = sparse_passes<32>(a, s); break;
    case 40: rc = sparse_passes<40>(a, s); break;
    case 48: rc = sparse_passes<48>(a, s); break;
    default: rc = sparse_passes<64>(a, s); break;
  }
  if (rc) return rc;
  hipLaunchKernelGGL(sp_finish_kernel, dim3((unsigned)((D * Lt + 255) / 256)), dim3(256), 0, s, a);
  GPZ_LAUNCH_OK();
  return 0;
}
